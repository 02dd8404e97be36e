/*
 * GpuTable.scala — `Table[GpuTable]` over the MI355X backend: the drop-in for
 * FlinkTable (flink-cypher/src/main/scala/org/opencypher/flink/impl/table/FlinkTable.scala:49-199).
 * Every SPI method is one JNI call (Native.scala → integration/jni/capf_jni.cpp
 * → include/capf_gpu.h).  Handles are immutable and reference counted: each
 * wrapper owns one reference, released by a Cleaner when it is unreachable.
 */
package org.opencypher.gpu

import java.lang.ref.Cleaner

import org.opencypher.okapi.api.types.CypherType
import org.opencypher.okapi.api.value.CypherValue._
import org.opencypher.okapi.impl.exception.{IllegalArgumentException, NotImplementedException}
import org.opencypher.okapi.ir.api.expr._
import org.opencypher.okapi.relational.api.table.Table
import org.opencypher.okapi.relational.impl.planning._
import org.opencypher.okapi.relational.impl.table.RecordHeader

object GpuTable {
  private val cleaner: Cleaner = Cleaner.create()

  private final class Release(handle: Long) extends Runnable {
    override def run(): Unit = Native.tableRelease(handle)
  }

  /** Takes ownership of a handle returned by a native call. */
  def apply(handle: Long)(implicit session: GpuCypherSession): GpuTable = new GpuTable(handle)

  def joinTypeCode(joinType: JoinType): Int = joinType match {   // PhysicalConstants.scala:29-35
    case InnerJoin => Native.JoinInner
    case LeftOuterJoin => Native.JoinLeftOuter
    case RightOuterJoin => Native.JoinRightOuter
    case FullOuterJoin => Native.JoinFullOuter
    case CrossJoin => Native.JoinCross
  }
}

final class GpuTable private (private[gpu] val handle: Long)(implicit val session: GpuCypherSession)
  extends Table[GpuTable] {

  GpuTable.cleaner.register(this, new GpuTable.Release(handle))

  private def wrap(h: => Long): GpuTable = GpuTable(Native.guard(h))

  // ---------------------------------------------------------------- CypherTable
  override def physicalColumns: Seq[String] = Native.guard(Native.tableColumns(handle)).toSeq  // CypherTable.scala:48

  override def columnType: Map[String, CypherType] =                                          // CypherTable.scala:58
    physicalColumns.map(c => c -> GpuTypes.toCypher(Native.guard(Native.tableColumnType(handle, c)))).toMap

  override def rows: Iterator[String => CypherValue] = GpuRows.download(this)                 // CypherTable.scala:63

  override def size: Long = Native.guard(Native.tableSize(handle))                            // CypherTable.scala:68

  // ---------------------------------------------------------------- Table[T]
  override def cache(): GpuTable = wrap(Native.tableCache(handle))                            // Table.scala:52

  override def select(col: (String, String), cols: (String, String)*): GpuTable = {         // Table.scala:71
    val all = col +: cols
    wrap(Native.tableSelect(handle, all.map(_._1).toArray, all.map(_._2).toArray))
  }

  override def filter(expr: Expr)(implicit header: RecordHeader, parameters: CypherMap): GpuTable = { // :81
    val (t, Seq(e2), h2, tmps) = hoistLists(Seq(expr), header, parameters)
    if (tmps.nonEmpty) return t.filter(e2)(h2, parameters).select(physicalColumns: _*)
    // (e2: a split of literals folded to a list literal)
    wrap(Native.tableFilter(handle, GpuExprMapper.program(e2, header, this, parameters)))
  }

  override def drop(cols: String*): GpuTable = wrap(Native.tableDrop(handle, cols.toArray))   // :89

  override def join(other: GpuTable, joinType: JoinType, joinCols: (String, String)*): GpuTable = { // :99
    // disjoint column sets, as FlinkTable.join asserts (FlinkTable.scala:173-174); the
    // backend raises CAPF_ERR_ILLEGAL_ARGUMENT for an overlap as well
    wrap(Native.tableJoin(handle, other.handle, GpuTable.joinTypeCode(joinType),
      joinCols.map(_._1).toArray, joinCols.map(_._2).toArray))
  }

  override def unionAll(other: GpuTable): GpuTable = wrap(Native.tableUnionAll(handle, other.handle)) // :107

  override def orderBy(sortItems: (Expr, Order)*)(implicit header: RecordHeader, parameters: CypherMap): GpuTable = // :115
    wrap(Native.tableOrderBy(handle,
      sortItems.map { case (e, _) => GpuExprMapper.program(e, header, this, parameters) }.toArray,
      sortItems.map { case (_, o) => o == Descending }.toArray))

  override def skip(n: Long): GpuTable = wrap(Native.tableSkip(handle, n))                   // :123

  override def limit(n: Long): GpuTable = wrap(Native.tableLimit(handle, n))                 // :131

  override def distinct: GpuTable = wrap(Native.tableDistinct(handle))                       // :138

  override def distinct(cols: String*): GpuTable = wrap(Native.tableDistinctCols(handle, cols.toArray)) // :146

  override def group(by: Set[Var], aggregations: Map[String, Aggregator])                      // :158-159
    (implicit header: RecordHeader, parameters: CypherMap): GpuTable = {
    // grouping columns: every column owned by a grouping var (FlinkTable.scala:129-135)
    val byCols = by.toSeq.flatMap(v => header.ownedBy(v).toSeq.map(header.column)).distinct
    val aggs = aggregations.toSeq
    val lowered = aggs.map { case (_, agg) => GpuExprMapper.aggregator(agg, header, this, parameters) }
    wrap(Native.tableGroupEx(handle, byCols.toArray, lowered.map(_._1).toArray, lowered.map(_._2).toArray,
      lowered.map(_._3).toArray, lowered.map(_._4).toArray, aggs.map(_._1).toArray))
  }

  /** The list-valued function expressions built by capf_table_list_fn (table.py
    * `_hoist_lists`): reverse, range, the three slices and an Add with a list side
    * (SparkSQLExprMapper.scala:171-182, 265, 269, 336-338), as (selector, arguments). */
  private def listFnArgs(e: Expr): Option[(Int, Seq[Option[Expr]])] = e match {
    case r: Reverse if r.expr.cypherType.material.isInstanceOf[CTList] || r.expr.cypherType.material == CTNull =>
      Some(Native.ListFnReverse -> Seq(Some(r.expr)))
    case r: Range => Some(Native.ListFnRange -> Seq(Some(r.from), Some(r.to), r.o))
    case s: ListSliceFromTo => Some(Native.ListFnSlice -> Seq(Some(s.list), Some(s.from), Some(s.to)))
    case s: ListSliceFrom => Some(Native.ListFnSlice -> Seq(Some(s.list), Some(s.from), None))
    case s: ListSliceTo => Some(Native.ListFnSlice -> Seq(Some(s.list), None, Some(s.to)))
    case a: Add if a.lhs.cypherType.material.isInstanceOf[CTList] || a.rhs.cypherType.material.isInstanceOf[CTList] =>
      Some(Native.ListFnConcat -> Seq(Some(a.lhs), Some(a.rhs)))
    case _ => None
  }

  /** A lambda expression over a list (okapi Expr.scala:199, 1178-1237; the Morpheus lowering
    * SparkSQLExprMapper.scala:340-395) as (CAPF_LAMBDA_* kind, list operand, predicate, body,
    * init, bound variables in slot order): table.py `lambda_parts`.  In reduce slot 0 is the
    * accumulator and slot 1 the element. */
  private def lambdaParts(e: Expr)
  : Option[(Int, Expr, Option[Expr], Option[Expr], Option[Expr], Seq[Expr])] = e match {
    case c: ListComprehension =>
      Some((Native.LambdaComprehension, c.expr, c.innerPredicate, c.extractExpression, None, Seq(c.variable)))
    case r: ListReduction =>
      Some((Native.LambdaReduce, r.list, None, Some(r.reduceExpr), Some(r.initExpr), Seq(r.accumulator, r.variable)))
    case f: ListFilter => Some((Native.LambdaComprehension, f.list, Some(f.predicate), None, None, Seq(f.variable)))
    case q: ListAny => Some((Native.LambdaAny, q.list, Some(q.predicate), None, None, Seq(q.variable)))
    case q: ListAll => Some((Native.LambdaAll, q.list, Some(q.predicate), None, None, Seq(q.variable)))
    case q: ListNone => Some((Native.LambdaNone, q.list, Some(q.predicate), None, None, Seq(q.variable)))
    case q: ListSingle => Some((Native.LambdaSingle, q.list, Some(q.predicate), None, None, Seq(q.variable)))
    case _ => None
  }

  /** Every list-valued sub-expression (listFnArgs; a lambda expression; a list literal of
    * per-row items below the top) projected to a temporary column, innermost first, and
    * replaced by a Var of that column: (table, rewritten expressions, header, temporaries).
    * A lambda expression has its list operand and init hoisted like any other argument and
    * its predicate / body compiled with the lambda variables bound
    * (capf_table_list_lambda); the temporary is a LIST for a comprehension or filter, a
    * scalar for a quantifier or reduce. */
  private def hoistLists(exprs: Seq[Expr], header: RecordHeader, parameters: CypherMap)
  : (GpuTable, Seq[Expr], RecordHeader, Seq[String]) = {
    var t = this
    var h = header
    var tmps = Vector.empty[String]
    var done = Map.empty[Expr, Expr]
    def tmp(): String = { tmps :+= s"\u0003lf${tmps.size}"; tmps.last }
    def perRowLiteral(e: Expr): Boolean = e match {
      case ListLit(items) => items.exists(i => !i.isInstanceOf[Lit[_]] && !i.isInstanceOf[Param])
      case _ => false
    }
    def columnFor(a: Expr): String =
      if (h.contains(a) && t.physicalColumns.contains(h.column(a))) h.column(a)
      else { val c = tmp(); t = t.withColumns(a -> c)(h, parameters); c }
    // what a lambda body may not hold (table.py `check_lambda_body`)
    def checkLambdaBody(x: Expr, owner: Expr): Unit = {
      val what = x match {
        case _ if lambdaParts(x).isDefined => Some("a lambda expression inside a lambda body (nested lists)")
        case _ if listFnArgs(x).isDefined => Some("a list-valued sub-expression inside a lambda body")
        case _ if perRowLiteral(x) => Some("a list literal of per-row items inside a lambda body")
        case _: Aggregator => Some("an aggregator inside a lambda body")
        case Rand => Some("rand() inside a lambda body")
        case _ => None
      }
      what.foreach(w => throw NotImplementedException(s"$w: $x in $owner"))
      if (!x.isInstanceOf[ListLit]) x.children.foreach(checkLambdaBody(_, owner))
    }
    def lowerLambda(e: Expr, kind: Int, list: Expr, pred: Option[Expr], body: Option[Expr], init: Option[Expr],
                    variables: Seq[Expr]): String = {
      import org.opencypher.okapi.api.types._
      (pred ++ body).foreach(checkLambdaBody(_, e))
      val listCol = columnFor(lower(list, top = false))
      val initCol = init.map(i => columnFor(lower(i, top = false))).getOrElse("")
      val slots = variables.zipWithIndex.map {
        case (v: Var, i) => v.name -> i
        case (other, _) => throw IllegalArgumentException("a lambda variable", other)
      }.toMap
      val elem = list.cypherType.material match { case CTList(inner) => inner; case _ => CTNull }
      val outType: CypherType = kind match {
        case Native.LambdaComprehension => body.map(_.cypherType).getOrElse(elem)
        case Native.LambdaReduce =>  // init's type; INTEGER with a FLOAT body widens; a NULL init takes the body's
          (init.get.cypherType.material, body.get.cypherType.material) match {
            case (CTNull | CTVoid, bt) => bt
            case (CTInteger, CTFloat) => CTFloat
            case (it, _) => it
          }
        case _ => CTBoolean
      }
      if (outType.material.isInstanceOf[CTList]) throw NotImplementedException(s"nested lists in $e")
      val c = tmp()
      val predProgram = pred.map(GpuExprMapper.program(_, h, t, parameters, slots)).orNull
      val bodyProgram = body.map(GpuExprMapper.program(_, h, t, parameters, slots)).orNull
      t = wrap(Native.tableListLambda(t.handle, kind, listCol, predProgram, bodyProgram, initCol,
        GpuTypes.fromCypher(outType), c))
      c
    }
    // split(s, d) (okapi Expr.scala:904-912; table.py `_str_split`): both literal — a list literal at
    // plan time; every distinct non-NULL delimiter plain — capf_table_str_split on the device string
    // heap; else (a regex, the empty delimiter, a lone surrogate) String.split(d, -1) per distinct pair
    // on the host and a column from host lists.
    def literalString(x: Expr): Option[Option[String]] = x match {
      case StringLit(v) => Some(Some(v))
      case NullLit(_) => Some(None)
      case Param(name) => parameters(name) match {
        case CypherString(v) => Some(Some(v))
        case CypherNull => Some(None)
        case _ => None
      }
      case _ => None
    }
    def lowerSplit(sp: Split): Either[Expr, String] = (literalString(sp.original), literalString(sp.delimiter)) match {
      case (Some(Some(s)), Some(Some(d))) =>
        Left(ListLit(GpuStringFunctions.split(s, d).map(StringLit(_)).toList))
      case (Some(a), Some(b)) if a.isEmpty || b.isEmpty => Left(NullLit())
      case _ =>
        import org.opencypher.okapi.api.types.CTString
        val strCol = columnFor(sp.original)
        val delimCol = columnFor(sp.delimiter)
        val typed = Seq(strCol, delimCol).forall(c => t.columnType(c) == CTString || t.columnType(c) == CTString.nullable)
        val pairs: Seq[(CypherValue, CypherValue)] =
          if (!typed) Seq.empty
          else GpuRows.download(t.select(strCol, delimCol)).map(r => (r(strCol), r(delimCol))).toSeq
        val onHost = pairs.exists {
          case (_, CypherString(d)) => !GpuStringFunctions.plainSplitDelimiter(d)
          case _ => false
        }
        val c = tmp()
        if (onHost && pairs.exists { case (CypherString(_), CypherString(_)) => true; case _ => false }) {
          val memo = scala.collection.mutable.Map.empty[(String, String), CypherValue]
          val lists = pairs.map {
            case (CypherString(s), CypherString(d)) =>
              memo.getOrElseUpdate((s, d), CypherList(GpuStringFunctions.split(s, d).map(CypherString(_)): _*))
            case _ => CypherNull
          }
          t = wrap(GpuRows.addList(t, c, lists))
        } else {
          t = wrap(Native.tableStrSplit(t.handle, strCol, delimCol, c))
        }
        Right(c)
    }
    def lower(e: Expr, top: Boolean): Expr = done.getOrElse(e, {
      val parts = lambdaParts(e)
      if (parts.isDefined) {
        val (kind, list, pred, body, init, variables) = parts.get
        val c = lowerLambda(e, kind, list, pred, body, init, variables)
        val v = Var(c)(e.cypherType)
        h = h.withExpr(v)
        if (h.column(v) != c) t = t.select(t.physicalColumns.map(x => if (x == c) c -> h.column(v) else x -> x): _*)
        done += e -> v
        v
      } else {
        val kids = e.children.map(c => lower(c, top = false))
        val e2 = if (kids.isEmpty || e.isInstanceOf[ListLit]) e else e.withNewChildren(kids.toArray)
        val folded: Option[Expr] = e2 match {
          case sp: Split => lowerSplit(sp) match {
            case Left(lit) => Some(lit)
            case Right(c) => Some(Var(c)(e2.cypherType))
          }
          case _ => None
        }
        val col: Option[String] = folded match {
          case Some(v: Var) => Some(v.name)
          case Some(_) => None
          case None => listFnArgs(e2) match {
          case Some((fn, args)) =>
            val names = args.map {
              case None => ""
              case Some(a) if h.contains(a) && t.physicalColumns.contains(h.column(a)) => h.column(a)
              case Some(a) => val c = tmp(); t = t.withColumns(a -> c)(h, parameters); c
            }
            val c = tmp()
            t = wrap(Native.tableListFn(t.handle, fn, names.toArray, c))
            Some(c)
          case None if !top && perRowLiteral(e2) =>
            val c = tmp(); t = t.withColumns(e2 -> c)(h, parameters); Some(c)
          case None => None
          }
        }
        col match {
          case Some(c) =>
            val v = Var(c)(e2.cypherType)
            h = h.withExpr(v)
            // the temporary is read under its own name
            if (h.column(v) != c) t = t.select(t.physicalColumns.map(x => if (x == c) c -> h.column(v) else x -> x): _*)
            done += e -> v
            v
          case None => folded.getOrElse(e2)
        }
      }
    })
    val out = exprs.map(lower(_, top = true))
    (t, out, h, tmps.map(c => if (h.contains(Var(c)())) h.column(Var(c)()) else c))
  }

  override def withColumns(columns: (Expr, String)*)(implicit header: RecordHeader, parameters: CypherMap): GpuTable = { // :170
    val (hoisted, exprs, h2, tmps) = hoistLists(columns.map(_._1), header, parameters)
    if (tmps.nonEmpty) {  // list functions: temporary LIST columns, dropped afterwards
      val out = hoisted.withColumns(exprs.zip(columns.map(_._2)): _*)(h2, parameters)
      return out.select(out.physicalColumns.filterNot(tmps.contains): _*)
    }
    if (exprs != columns.map(_._1))  // a split of literals folded: no temporary
      return withColumns(exprs.zip(columns.map(_._2)): _*)
    val (literalLists, others) = columns.partition { case (e, _) => listItems(e, parameters).isDefined }
    if (literalLists.nonEmpty) {  // [x, y, ...] / $list (FlinkSQLExprMapper.scala:71, 75): capf_table_list_columns
      val base = if (others.isEmpty) this else withColumns(others: _*)
      val keep = base.physicalColumns
      val built = literalLists.zipWithIndex.foldLeft(base) { case (t, ((e, col), i)) =>
        val items = listItems(e, parameters).get
        val tmp = items.indices.map(j => s"\u0003le$i.$j")
        val withItems = if (items.isEmpty) t else t.withColumns(items.zip(tmp): _*)
        wrap(Native.tableListColumns(withItems.handle, tmp.toArray, col))
      }
      return built.select(keep ++ literalLists.map(_._2): _*)
    }
    val (lists, rest) = columns.partition { case (e, _) => e.isInstanceOf[Labels] || e.isInstanceOf[Keys] }
    val (explodes, plain) = rest.partition { case (e, _) => e.isInstanceOf[Explode] }
    val base =
      if (plain.isEmpty) this
      else wrap(Native.tableWithColumns(handle,
        plain.map { case (e, _) => GpuExprMapper.program(e, header, this, parameters) }.toArray,
        plain.map(_._2).toArray))
    val withLists = lists.foldLeft(base) { case (t, (e, col)) => t.nameList(e, col, header) }
    explodes.foldLeft(withLists) { case (t, (Explode(list), col)) => t.explode(list, col, header, parameters) }
  }

  /** The element expressions of a list literal, or of a parameter holding a list. */
  private def listItems(e: Expr, parameters: CypherMap): Option[Seq[Expr]] = e match {
    case ListLit(items) => Some(items)
    case Param(p) => parameters.value.get(p) match {
      case Some(CypherList(vs)) => Some(vs.map {
        case CypherNull => NullLit()
        case CypherInteger(v) => IntegerLit(v)
        case CypherFloat(v) => FloatLit(v)
        case CypherString(v) => StringLit(v)
        case CypherBoolean(v) => if (v) TrueLit else FalseLit
        case other => throw NotImplementedException(s"GPU list element $other")
      })
      case _ => None
    }
    case _ => None
  }

  /** labels(n) / keys(n) (FlinkSQLExprMapper.scala:136-153): the label flag columns
    * (TRUE) or property columns (any value) of n, sorted by name, as a LIST<STRING>
    * column.  keys lists every property holding a value (GetKeys, :321-329, matches
    * `case (key, true)` on the VALUE — a reference bug not reproduced). */
  private def nameList(e: Expr, col: String, header: RecordHeader): GpuTable = {
    val present = physicalColumns.toSet
    val (found, kind) = e match {
      case Labels(v) => (header.labelsFor(v.owner.get).toSeq.map(l => l.label.name -> header.column(l)), 0)
      case Keys(v) => (header.propertiesFor(v.owner.get).toSeq.map(p => p.key.name -> header.column(p)), 1)
      case other => throw NotImplementedException(s"GPU list function $other")
    }
    val cols = found.filter { case (_, c) => present(c) }.sortBy(_._1)
    wrap(Native.tableNameList(handle, cols.map(_._2).toArray, Array.fill(cols.size)(kind),
      cols.map { case (n, _) => session.intern(n) }.toArray, col))
  }

  /** UNWIND list AS item = add(Explode(list) as item) (RelationalPlanner.scala:99-101). */
  private def explode(list: Expr, col: String, header: RecordHeader, parameters: CypherMap): GpuTable = {
    val literal: Option[Seq[CypherValue]] = list match {
      case ListLit(items) => Some(items.map {
        case NullLit(_) => CypherNull
        case IntegerLit(v) => CypherInteger(v)
        case FloatLit(v) => CypherFloat(v)
        case StringLit(v) => CypherString(v)
        case TrueLit => CypherBoolean(true)
        case FalseLit => CypherBoolean(false)
        case Param(p) => parameters(p)
        case other => throw NotImplementedException(s"GPU UNWIND element $other")
      })
      case Param(p) => parameters(p) match {
        case CypherList(vs) => Some(vs)
        case CypherNull => Some(Seq.empty)
        case other => throw NotImplementedException(s"GPU UNWIND of $other")
      }
      case NullLit(_) => Some(Seq.empty)
      case _ => None
    }
    literal match {
      case Some(vs) => wrap(GpuRows.explodeValues(this, col, vs))
      case None if header.contains(list) => wrap(Native.tableExplodeList(handle, header.column(list), col))
      case None => throw NotImplementedException(s"GPU UNWIND of $list")
    }
  }

  override def show(rows: Int): Unit = Native.guard(Native.tableShow(handle, rows))        // :177

  // ---------------------------------------------------------------- beyond the SPI
  /** Count into device memory without the host wait (capf_table_count_async). */
  def countAsync(dCount: Long): Unit = Native.guard(Native.tableCountAsync(handle, dCount))

  /** Re-encode INTEGER columns narrower (FOR32 / FOR24); values unchanged. */
  def compact(width: Int = 4): GpuTable = wrap(Native.tableCompactWidth(handle, width))
}

object GpuTypes {
  import org.opencypher.okapi.api.types._

  /** FlinkConversions.scala:43-117: LONG → CTInteger, DOUBLE → CTFloat, … (nullable: the
    * backend tracks validity per column, FlinkTable reports nullable types too). */
  def toCypher(code: Int): CypherType = code match {
    case Native.TypeInt64 => CTInteger.nullable
    case Native.TypeFloat64 => CTFloat.nullable
    case Native.TypeBool => CTBoolean.nullable
    case Native.TypeString => CTString.nullable
    case Native.TypeNull => CTNull
    case Native.TypeList => CTList(CTAny).nullable   // element type: Native.tableListInfo
    case other => throw IllegalArgumentException("a capf column type", other)
  }

  def fromCypher(t: CypherType): Int = t.material match {
    case CTInteger | _: CTNode | _: CTRelationship | CTIdentity => Native.TypeInt64
    case CTFloat => Native.TypeFloat64
    case CTBoolean => Native.TypeBool
    case CTString => Native.TypeString
    case CTNull | CTVoid => Native.TypeNull
    case other => throw org.opencypher.okapi.impl.exception.NotImplementedException(s"GPU column of type $other")
  }
}
