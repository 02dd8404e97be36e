/*
 * capf_gpu.h — C-ABI of the MI355X relational backend for okapi-relational.
 *
 * This is the drop-in boundary that replaces the Flink implementation of the
 * okapi `Table[T]` SPI.  Every entry point below corresponds to one method of
 *
 *   trait Table[T <: Table[T]] extends CypherTable
 *     okapi-relational/src/main/scala/org/opencypher/okapi/relational/api/table/Table.scala:43-178
 *   trait CypherTable
 *     okapi-api/src/main/scala/org/opencypher/okapi/api/table/CypherTable.scala:41-70
 *
 * as implemented today by FlinkTable
 *     flink-cypher/src/main/scala/org/opencypher/flink/impl/table/FlinkTable.scala:49-199
 *
 * (citations are relative to the reference checkout).  A JVM shim
 * (`GpuTable extends Table[GpuTable]`) binds these
 * functions 1:1 over JNI; the Python host layer in
 * cypher-for-apache-flink_amd/table.py binds them over ctypes.
 *
 * Conventions
 *  - Tables are immutable, reference-counted handles.  Every operation returns
 *    a NEW handle (Table.scala: "every op returns a new T"); the caller owns it
 *    and must capf_table_release() it.  Column buffers are shared between
 *    handles, so select/drop/alias are metadata-only.
 *  - Evaluation is lazy, exactly like the Flink Table API: operations build a
 *    plan DAG; nothing runs on the GPU until capf_table_size / capf_table_download
 *    (FlinkTable.scala:57-61, CAPFRecords.scala:142-144).  This is what lets
 *    `group(∅, count(*))` over an Expand join chain run as a fused,
 *    factorised count instead of materialising ~1e12 joined rows.
 *  - Every function returns CAPF_OK (0) or a negative status.  The message
 *    is available from capf_last_error() (thread-local) and the kind from
 *    capf_last_error_kind(); the shim rethrows the matching
 *    okapi.impl.exception (okapi-api/.../impl/exception/InternalException.scala:36-65).
 *  - Column names are arbitrary caller strings (RecordHeader column names,
 *    okapi-relational/.../impl/table/RecordHeader.scala:299-318).
 *  - Logical types follow the Flink type mapping
 *    (flink-cypher/.../impl/convert/FlinkConversions.scala:43-117):
 *    CTInteger / node / relationship ids → INT64, CTFloat → FLOAT64,
 *    CTBoolean → BOOL, CTString → STRING (dictionary codes, see capf_string_*).
 */
#ifndef CAPF_GPU_H
#define CAPF_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAPF_ABI_VERSION 1

typedef struct capf_session capf_session;
typedef struct capf_table capf_table;
typedef int32_t capf_status;

/* status codes */
enum {
  CAPF_OK = 0,
  CAPF_ERR_ILLEGAL_ARGUMENT = -1, /* okapi IllegalArgumentException */
  CAPF_ERR_NOT_IMPLEMENTED = -2,  /* okapi NotImplementedException   */
  CAPF_ERR_INTERNAL = -3,         /* okapi IllegalStateException / InternalException */
  CAPF_ERR_HIP = -4,              /* HIP runtime failure               */
  CAPF_ERR_OOM = -5               /* device allocation failed          */
};

/* column types (FlinkConversions.scala:43-117) */
enum {
  CAPF_TYPE_NULL = 0,    /* CTNull: column of nulls */
  CAPF_TYPE_INT64 = 1,   /* CTInteger, CTNode/CTRelationship/CTIdentity ids (Types.LONG) */
  CAPF_TYPE_FLOAT64 = 2, /* CTFloat (Types.DOUBLE) */
  CAPF_TYPE_BOOL = 3,    /* CTBoolean, HasLabel / HasType columns */
  CAPF_TYPE_STRING = 4,  /* CTString, stored as int64 dictionary codes */
  CAPF_TYPE_LIST = 5,    /* CTList(elem): the result of collect (see capf_table_list_info) */
  /* CTDate / CTLocalDateTime: an int64 payload like STRING's codes — days since
   * 1970-01-01 / microseconds since 1970-01-01T00:00:00, negative before the
   * epoch; no time zone, no nanoseconds (DESIGN.md "Temporal values").  Every
   * operation that treats a column as plain int64 (upload, download, filter,
   * union, sort, group / distinct keys, joins on equal-typed keys, MIN / MAX /
   * COUNT, skip / limit, the FOR encodings) takes them down the INTEGER path and
   * keeps the type; SUM / AVG / stDev / percentiles are IllegalArgument, collect
   * and LIST elements NotImplemented.                                         */
  CAPF_TYPE_DATE = 6,
  CAPF_TYPE_LOCALDATETIME = 7
};

/* join types (okapi-relational/.../impl/planning/PhysicalConstants.scala:29-35) */
enum {
  CAPF_JOIN_INNER = 0,
  CAPF_JOIN_LEFT_OUTER = 1,
  CAPF_JOIN_RIGHT_OUTER = 2,
  CAPF_JOIN_FULL_OUTER = 3,
  CAPF_JOIN_CROSS = 4
};

/* aggregators (okapi-ir/.../api/expr/Expr.scala:1031-1140,
 * lowered as in FlinkSQLExprMapper.scala:281-287) */
enum {
  CAPF_AGG_COUNT_STAR = 0,
  CAPF_AGG_COUNT = 1,
  CAPF_AGG_SUM = 2,
  CAPF_AGG_MIN = 3,
  CAPF_AGG_MAX = 4,
  CAPF_AGG_AVG = 5,
  /* Collect (Expr.scala Collect; Flink child0.collect, FlinkSQLExprMapper.scala:283):
   * the non-NULL values of each group as a LIST column (empty list for none);
   * agg_distinct drops duplicate values.  Flink's COLLECT is a MULTISET: the
   * element order is not part of the result (here: ascending values, string
   * elements in dictionary-code order). */
  CAPF_AGG_COLLECT = 6,
  /* StDev / StDevP (Expr.scala:1120-1128; Flink child0.stddevSamp / stddevPop,
   * FlinkSQLExprMapper.scala:223-224): the sample / population standard
   * deviation of the group's non-NULL numeric values as a FLOAT; NULL for a
   * group without values (AggregationTests.scala:610-617, 637-644) and, for
   * the sample form, with one value (Calcite's STDDEV_SAMP divides by
   * count - 1 and yields NULL for count = 1).  Two-pass, double-double sums. */
  CAPF_AGG_STDEV = 7,
  CAPF_AGG_STDEV_POP = 8,
  /* PercentileCont / PercentileDisc (Expr.scala:1096-1118) with the fraction
   * p = agg_params[i] in [0, 1] of capf_table_group_ex.  The semantics of the
   * Spark backend of the same SPI (morpheus-spark-cypher/.../impl/expressions/
   * PercentileUdafs.scala:59-96; Flink has no mapping): over the sorted
   * non-NULL values v[0..n), disc = v[max(round(n·p), 1) − 1] in the input's
   * type; cont = linear interpolation at position 1 + (n − 1)·p, a FLOAT.
   * NULL for a group without values.                                        */
  CAPF_AGG_PERCENTILE_CONT = 9,
  CAPF_AGG_PERCENTILE_DISC = 10
};

/*
 * Expression programs.  The shim lowers the supported subset of okapi `Expr`
 * trees (what FlinkSQLExprMapper.asFlinkSQLExpr handles,
 * flink-cypher/.../impl/FlinkSQLExprMapper.scala:48-294) into a postfix
 * program evaluated per row on the GPU with Cypher three-valued logic.
 * Parameters (`Param`) are substituted as literals by the shim.
 */
enum {
  CAPF_OP_COL = 1,         /* push column names[iarg]                       */
  CAPF_OP_LIT_INT = 2,     /* push int64 iarg                               */
  CAPF_OP_LIT_FLOAT = 3,   /* push double farg                              */
  CAPF_OP_LIT_BOOL = 4,    /* push bool iarg != 0                           */
  CAPF_OP_LIT_STRING = 5,  /* push string code iarg (capf_string_intern)    */
  CAPF_OP_LIT_NULL = 6,    /* push NULL of capf type iarg                   */
  CAPF_OP_EQ = 10,         /* Equals            (===)                       */
  CAPF_OP_NEQ = 11,        /* Not(Equals)       fused                       */
  CAPF_OP_LT = 12,         /* LessThan                                      */
  CAPF_OP_LE = 13,         /* LessThanOrEqual                               */
  CAPF_OP_GT = 14,         /* GreaterThan                                   */
  CAPF_OP_GE = 15,         /* GreaterThanOrEqual                            */
  CAPF_OP_NOT = 20,        /* Not                                           */
  CAPF_OP_AND = 21,        /* Ands, arity iarg                              */
  CAPF_OP_OR = 22,         /* Ors,  arity iarg                              */
  CAPF_OP_IS_NULL = 23,    /* IsNull                                        */
  CAPF_OP_IS_NOT_NULL = 24,/* IsNotNull / Exists                            */
  CAPF_OP_ADD = 30,        /* Add (numeric)                                 */
  CAPF_OP_SUB = 31,        /* Subtract                                      */
  CAPF_OP_MUL = 32,        /* Multiply                                      */
  CAPF_OP_DIV = 33,        /* Divide (integer division on int64 operands)   */
  CAPF_OP_MOD = 34,        /* Modulo                                        */
  CAPF_OP_NEG = 35,        /* unary minus                                   */
  CAPF_OP_TO_FLOAT = 40,   /* ToFloat  → DOUBLE                             */
  CAPF_OP_TO_INTEGER = 41, /* ToInteger → Flink casts to INT (32-bit!)      */
  CAPF_OP_COALESCE = 50,   /* Coalesce, arity iarg                          */
  CAPF_OP_STR_LEN = 60,    /* Size(string): pop a STRING, push its length in
                              UTF-16 units (Java String.length, Flink
                              charLength, FlinkSQLExprMapper.scala:80-85)   */
  CAPF_OP_LIST_SIZE = 61,  /* Size(list): push the element count of LIST
                              column names[iarg] (Flink cardinality, :80-85) */
  CAPF_OP_IF = 62,         /* pop value, cond, else: push cond TRUE ? value :
                              else (type(r) over the HasType columns,
                              FlinkSQLExprMapper.scala:152-160; CaseExpr
                              as a chain of Ifs, :242-260); numeric branches
                              of different types widen to FLOAT             */
  /* Mathematical functions (FlinkSQLExprMapper.scala:199-221).  Unary: pop x,
   * push f(x); NULL in, NULL out.  ROUND rounds half away from zero and
   * yields a FLOAT (the Spark mapping round(x).cast(Double),
   * SparkSQLExprMapper.scala:286; Flink's is `???`); CEIL / FLOOR yield
   * FLOAT for FLOAT input, INTEGER input unchanged; SIGN an INTEGER; ABS
   * keeps the type; the rest FLOAT (Java Math.* over doubles).               */
  CAPF_OP_ROUND = 70,
  CAPF_OP_ABS = 71,
  CAPF_OP_CEIL = 72,
  CAPF_OP_FLOOR = 73,
  CAPF_OP_SIGN = 74,
  CAPF_OP_SQRT = 75,
  CAPF_OP_LOG = 76,
  CAPF_OP_LOG10 = 77,
  CAPF_OP_EXP = 78,
  CAPF_OP_SIN = 79,
  CAPF_OP_COS = 80,
  CAPF_OP_TAN = 81,
  CAPF_OP_ASIN = 82,
  CAPF_OP_ACOS = 83,
  CAPF_OP_ATAN = 84,
  CAPF_OP_DEGREES = 85,
  CAPF_OP_RADIANS = 86,
  CAPF_OP_ATAN2 = 87,      /* binary: pop x, y; push atan2(y, x)             */
  /* ToBoolean (:185, Flink cast to BOOLEAN): BOOLEAN unchanged, STRING
   * 'true' / 'false' (any case, trimmed) → TRUE / FALSE, any other string
   * → NULL.  Uses the session's device table of string → boolean codes.     */
  CAPF_OP_TO_BOOLEAN = 88,
  /* x IN [list] over a long INTEGER / STRING list (FlinkSQLExprMapper.scala:
   * 114-118 lowers IN to Flink's `in`): pops x; pushes TRUE when x is in the
   * session literal set names[i] (capf_session_literal_set, referenced as
   * "\x01set:<id>"), else NULL when x is NULL or farg != 0 (the list held a
   * NULL), else FALSE.  One binary search per row over the sorted set.       */
  CAPF_OP_IN_SET = 89,
  /* String functions of one STRING operand and literal arguments (toUpper /
   * toLower / trim / lTrim / rTrim / substring / replace / concatenation with
   * a literal, FlinkSQLExprMapper.scala:120-128, 187-195): pops a STRING code
   * c; pushes entry c of the code map names[iarg] — the function applied to
   * dictionary string c by the caller and interned (capf_session_code_map,
   * referenced as "\x01map:<id>"); NULL in, an entry < 0 (a NULL result) or
   * c past the map → NULL.                                                   */
  CAPF_OP_STR_MAP = 90,
  /* A new STRING per value (toString of an INTEGER / FLOAT column, the
   * concatenation of two columns, :120-128, :184): pops x (farg == 0) or
   * y then x (farg != 0); pushes the code of the value map names[iarg] entry
   * whose key is x's value (INTEGER / STRING code) or bit pattern (FLOAT), or
   * the key pair (x, y); NULL in or no entry → NULL.  The caller evaluated the
   * operands' distinct values, built their strings and interned them
   * (capf_session_value_map, "\x01vmap:<id>").                                */
  CAPF_OP_VALUE_MAP = 91,
  /* toFloat / toInteger of a STRING (FlinkSQLExprMapper.scala:182-183, CAST
   * to DOUBLE / INT): pops a STRING code; iarg 1 pushes it parsed as a
   * DOUBLE (Java Double.valueOf grammar after trim: decimal / exponent forms,
   * NaN, Infinity, an f / d suffix), iarg 0 as an INTEGER (a decimal integer,
   * a fractional part truncated, within 32 bits).  An unparsable string (or
   * NULL) pushes NULL.  Uses the session's device table of parsed strings.   */
  CAPF_OP_STR_TO_NUM = 92,
  /* rand() (:207): pushes a uniform DOUBLE in [0, 1) — splitmix64 of
   * (iarg seed, row); the caller draws a fresh seed per evaluation.          */
  CAPF_OP_RAND = 93,
  /* xs[i] on a LIST column (ContainerIndex, :262-269): pops an INTEGER i;
   * pushes element i of the row's list in LIST column names[iarg] (i < 0
   * counts from the end); NULL for a NULL list, a NULL index or an index out
   * of range.  farg = the element's capf type (CAPF_TYPE_*).                 */
  CAPF_OP_LIST_INDEX = 94,
  /* Ordering of strings (Flink compares VARCHARs lexicographically, Java
   * String.compareTo; FlinkSQLExprMapper.scala:91-94 and ORDER BY): pops a
   * STRING; pushes its INTEGER rank among the session's strings in UTF-16
   * code-unit order, so <, <=, >, >= and sorting on ranks order the strings.
   * NULL in, NULL out.  capf_table_order_by applies it to a STRING key itself. */
  CAPF_OP_STR_RANK = 95,
  /* STARTS WITH / ENDS WITH / CONTAINS (okapi Expr.scala:369-379; Flink's
   * mapper raises NotImplemented for the three, FlinkSQLExprMapper.scala:
   * 96-98): pops the pattern, then the subject (both STRING); pushes a
   * BOOLEAN.  iarg is the kind: 0 STARTS WITH, 1 ENDS WITH, 2 CONTAINS.  A
   * NULL operand gives NULL.  Matching is on the strings' UTF-8 bytes in the
   * session's device string heap (equal to matching code points); an empty
   * pattern matches every subject.  A literal pattern is answered from a
   * device table per dictionary string when that examines no more strings
   * than the input has rows, else row by row.                               */
  CAPF_OP_STR_MATCH = 96,
  /* x IN xs, xs a LIST column (okapi In; Morpheus array_contains,
   * SparkSQLExprMapper.scala:161-164; expectations NullTests.scala:127-132):
   * pops x; pushes the three-valued answer from a scan of the row's elements
   * in LIST column names[iarg] (farg = the element's capf type, as for
   * CAPF_OP_LIST_INDEX).  In this order: a NULL list gives NULL; an empty
   * list FALSE (for a NULL x too); a NULL x NULL; a non-NULL element equal
   * to x (CAPF_OP_EQ's equality, INTEGER and FLOAT numerically) TRUE;
   * otherwise NULL when the list holds a NULL element, else FALSE.  An element
   * type that cannot equal x's type gives NULL.                              */
  CAPF_OP_IN_LIST = 97,
  /* The bound variable of a lambda expression (okapi LambdaVar,
   * Expr.scala:199): pushes lambda slot iarg (0 or 1) of the evaluation.
   * Only the programs given to capf_table_list_lambda may hold it: slot 0 is
   * the list element (REDUCE: the accumulator), slot 1 REDUCE's element.
   * Anywhere else it is IllegalArgument.                                      */
  CAPF_OP_LAMBDA = 98,
  /* A DATE / LOCALDATETIME literal: pushes iarg (days / microseconds since the
   * epoch) typed farg (CAPF_TYPE_DATE or CAPF_TYPE_LOCALDATETIME).             */
  CAPF_OP_LIT_TEMPORAL = 99,
  /* d.year, ldt.hour, ... (okapi DateProperty / LocalDateTimeProperty; the
   * Morpheus temporalAccessor, TemporalConversions.scala:155-173): pops a DATE
   * or LOCALDATETIME, pushes field iarg (CAPF_TEMPORAL_*) as an INTEGER; NULL
   * in, NULL out.  A time field of a DATE is IllegalArgument.                 */
  CAPF_OP_TEMPORAL_FIELD = 100,
  /* temporal + duration: pops a DATE or LOCALDATETIME, pushes it moved by farg
   * months (an integer, exact in a double) and iarg microseconds; NULL in,
   * NULL out.  The months go first, by java.time's plusMonths (the day of
   * month clamped to the target month's length).  A DATE then moves by
   * iarg / 86 400 000 000 days, truncated toward zero (sub-day parts dropped,
   * TemporalUdfs.scala:46-88); a LOCALDATETIME has its date part moved by the
   * months and iarg added.  Subtraction is the caller negating both.          */
  CAPF_OP_TEMPORAL_ADD = 101
};

/* fields of CAPF_OP_TEMPORAL_FIELD: ISO-8601 calendar (java.time), the week
 * fields of the week-based year, DAY_OF_WEEK Monday = 1; 0..8 on both types,
 * 9..13 on a LOCALDATETIME only                                             */
enum {
  CAPF_TEMPORAL_YEAR = 0,
  CAPF_TEMPORAL_QUARTER = 1,
  CAPF_TEMPORAL_MONTH = 2,
  CAPF_TEMPORAL_WEEK = 3,
  CAPF_TEMPORAL_WEEK_YEAR = 4,
  CAPF_TEMPORAL_DAY_OF_QUARTER = 5,
  CAPF_TEMPORAL_DAY = 6,
  CAPF_TEMPORAL_ORDINAL_DAY = 7,
  CAPF_TEMPORAL_DAY_OF_WEEK = 8,
  CAPF_TEMPORAL_HOUR = 9,
  CAPF_TEMPORAL_MINUTE = 10,
  CAPF_TEMPORAL_SECOND = 11,
  CAPF_TEMPORAL_MILLISECOND = 12,
  CAPF_TEMPORAL_MICROSECOND = 13
};

typedef struct capf_expr {
  int32_t n;                 /* number of instructions                     */
  const int32_t *ops;        /* opcode per instruction                     */
  const int64_t *iargs;      /* integer immediate per instruction          */
  const double *fargs;       /* float immediate per instruction (may be 0) */
  int32_t n_names;           /* column names referenced by CAPF_OP_COL     */
  const char *const *names;
} capf_expr;

/* ---------------------------------------------------------------- errors */
const char *capf_last_error(void);
int32_t capf_last_error_kind(void);
int32_t capf_abi_version(void);

/* --------------------------------------------------------------- session
 * RelationalCypherSession[T] backend state
 * (okapi-relational/.../api/graph/RelationalCypherSession.scala:63-111;
 *  CAPFSession.create, flink-cypher/.../api/CAPFSession.scala:74-91).
 * `hip_stream` may be NULL (the session creates its own stream) or a
 * hipStream_t owned by the caller (e.g. torch.cuda.current_stream()).     */
capf_status capf_session_create(int32_t device, void *hip_stream, capf_session **out);
capf_status capf_session_destroy(capf_session *s);
capf_status capf_session_sync(capf_session *s);
/* Per-kernel HIP-event timing of the hot kernels (off by default).  reset also
 * sets the last plan back to "none". */
capf_status capf_session_set_profiling(capf_session *s, int32_t enabled);
capf_status capf_session_reset_profile(capf_session *s);
capf_status capf_session_profile_count(capf_session *s, int32_t *n);
capf_status capf_session_profile_entry(capf_session *s, int32_t i, const char **kernel,
                                       int64_t *launches, double *total_ms, double *bytes);
/* last fused execution path taken ("fused_chain2", "fused_triangle", "message_passing",
 * "message_passing_grouped" (group(keys of one leaf; count(*)) over an inner-join tree:
 * that leaf is the root and keeps one weight per row),
 * "fused_var_length_reach" (lower bound 0 / 1: BFS), "fused_var_length_trails"
 * (lower bound >= 2: trail enumeration), "fused_var_length_undirected" (undirected
 * pattern: step enumeration); "none" until one runs) */
const char *capf_session_last_plan(capf_session *s);
/* the messages and root kernel of the last "message_passing" count (DESIGN.md "Plan detail"); "" until one runs.
 * "message_passing_grouped" uses the same grammar per term with the root token "rows:<nchild>",
 * "rows1:<kind>:w<3|4|8>" or "rows_all", and ends in " group:unique" (every surviving row of the
 * group leaf is its own group) or " group:hash" (the rows are grouped, their weights summed) */
const char *capf_session_last_plan_detail(capf_session *s);

/* String dictionary for CAPF_TYPE_STRING columns. */
capf_status capf_string_intern(capf_session *s, const char *str, int64_t *code);
capf_status capf_string_lookup(capf_session *s, int64_t code, const char **str);
/* Size and FNV-1a digest of the dictionary in code order: ranks that exchange
 * STRING columns as codes check that their dictionaries agree (dist_table.py). */
capf_status capf_string_digest(capf_session *s, int64_t *count, uint64_t *digest);

/* ---------------------------------------------------- table construction
 * CAPFElementTable.create / CAPFRecordsFactory.from
 * (flink-cypher/.../api/io/CAPFTable.scala:76-83, impl/CAPFRecords.scala:47-100).
 * data[i]: nrows values of 8 bytes (INT64/FLOAT64/STRING) or 1 byte (BOOL),
 *          NULL for a CAPF_TYPE_NULL column.
 * valid[i]: NULL (no nulls) or nrows bytes, 1 = value present.            */
capf_status capf_table_from_host(capf_session *s, int32_t ncols, const char *const *names,
                                 const int32_t *types, const void *const *data,
                                 const uint8_t *const *valid, int64_t nrows, capf_table **out);
/* Same with device pointers; copy = 0 borrows them (caller keeps them alive). */
capf_status capf_table_from_device(capf_session *s, int32_t ncols, const char *const *names,
                                   const int32_t *types, void *const *data,
                                   uint8_t *const *valid, int64_t nrows, int32_t copy,
                                   capf_table **out);
/* RelationalCypherRecordsFactory.unit / empty(header)
 * (okapi-relational/.../api/table/RelationalCypherRecords.scala:43-54)       */
capf_status capf_table_unit(capf_session *s, capf_table **out);
capf_status capf_table_empty(capf_session *s, int32_t ncols, const char *const *names,
                             const int32_t *types, capf_table **out);
capf_status capf_table_retain(capf_table *t);
capf_status capf_table_release(capf_table *t);

/* ------------------------------------------------------------ CypherTable */
/* physicalColumns (CypherTable.scala:48) */
capf_status capf_table_num_columns(capf_table *t, int32_t *n);
capf_status capf_table_column_name(capf_table *t, int32_t i, const char **name);
/* physicalColumns in one call: *joined points at *bytes bytes holding the
 * *n column names, each terminated by '\0' (valid while the table lives)   */
capf_status capf_table_columns(capf_table *t, const char **joined, int64_t *bytes, int32_t *n);
/* columnType (CypherTable.scala:58) */
capf_status capf_table_column_type(capf_table *t, const char *col, int32_t *type);
/* size (CypherTable.scala:68): triggers execution */
capf_status capf_table_size(capf_table *t, int64_t *n);
/* size / group(∅, {count(*)}) without the host wait: the count lands in the
 * device int64 at d_count, ordered on the session stream.  Same value as
 * capf_table_size (CypherTable.scala:68) / the count(*) column of
 * Table.group (Table.scala:158-159); lets a driver plan query i+1 while the
 * GPU runs query i.  Shapes that are not a fused count fall back to the
 * synchronous count (then copy it to d_count).                             */
capf_status capf_table_count_async(capf_table *t, int64_t *d_count);
/* rows (CypherTable.scala:63): download one column; values buffer holds
 * size × (8 or 1) bytes, valid_out (may be NULL) size bytes.              */
capf_status capf_table_download(capf_table *t, const char *col, void *values_out,
                                uint8_t *valid_out);
/* LIST columns (CAPF_TYPE_LIST, from CAPF_AGG_COLLECT).  capf_table_list_info:
 * the element type (CAPF_TYPE_*) and the total element count of column col
 * (n_values NULL: the type alone, read off the plan without evaluating the
 * table whenever the plan determines it — collect, a list literal, labels /
 * keys, or a column passed through select / filter / join / union / sort).
 * capf_table_download_list: offsets_out[size + 1] (int64, list i = elements
 * [offsets[i], offsets[i+1])), values_out[n_values] elements (8 or 1 bytes
 * each; a NULL element's slot holds 0), valid_out[size] list validity (may
 * be NULL).  A list whose elements are all NULL-typed (`[null, null]`) has
 * element type CAPF_TYPE_NULL with n_values > 0: its offsets give its length,
 * nothing is written to values_out.
 * capf_table_download_list_nulls: which elements are NULL.  *has_nulls = 0
 * when the element column carries no validity and is not NULL-typed (nothing
 * is written); otherwise 1 and elem_valid_out[n_values] (1 = present, all 0
 * for NULL-typed elements).  elem_valid_out may be NULL: *has_nulls alone.
 * capf_table_download of a LIST column is CAPF_ERR_ILLEGAL_ARGUMENT.        */
capf_status capf_table_list_info(capf_table *t, const char *col, int32_t *elem_type,
                                 int64_t *n_values);
capf_status capf_table_download_list(capf_table *t, const char *col, int64_t *offsets_out,
                                     void *values_out, uint8_t *valid_out);
capf_status capf_table_download_list_nulls(capf_table *t, const char *col, uint8_t *elem_valid_out,
                                           int32_t *has_nulls);
/* Device view of a materialised column (for zero-copy interop). */
capf_status capf_table_device_column(capf_table *t, const char *col, void **values,
                                     uint8_t **valid, int64_t *nrows);

/* Storage encodings of a materialised column.  CAPF_ENC_FOR32: INTEGER values
 * held as uint32 offsets from a per-column base (frame of reference) — same
 * values, half the HBM bytes.  No reference counterpart: the Flink backend
 * stores ids as Java longs (CAPFGraph.scala ids are LongType).              */
#define CAPF_ENC_PLAIN 0
#define CAPF_ENC_FOR32 1
#define CAPF_ENC_FOR24 2 /* 3-byte offsets (range < 2^24): 3 B per id */
/* Materialise t and re-encode every INTEGER column whose value range spans
 * < 2^32 as FOR32.  Results of every operator are unchanged.               */
capf_status capf_table_compact(capf_table *t, capf_table **out);
/* The same with a narrowest width: 3 = FOR24 where the range spans < 2^24
 * (FOR32 where it only fits 32 bits), 4 = capf_table_compact.             */
capf_status capf_table_compact_width(capf_table *t, int32_t width, capf_table **out);
capf_status capf_table_column_encoding(capf_table *t, const char *col, int32_t *enc,
                                       int64_t *base);

/* --------------------------------------------------------------- Table[T] */
/* cache() (Table.scala:52) */
capf_status capf_table_cache(capf_table *t, capf_table **out);
/* Not an SPI method: evaluates the lazy operator DAG of t into device
 * memory (what rows / size do before their download or count) — the
 * materialising path timed by bench.py --query one_hop_rows.               */
capf_status capf_table_materialize(capf_table *t);
/* select((col, alias)+) (Table.scala:71) */
capf_status capf_table_select(capf_table *t, int32_t n, const char *const *cols,
                              const char *const *aliases, capf_table **out);
/* filter(expr)(header, params) (Table.scala:81) */
capf_status capf_table_filter(capf_table *t, const capf_expr *pred, capf_table **out);
/* drop(cols*) (Table.scala:89) */
capf_status capf_table_drop(capf_table *t, int32_t n, const char *const *cols, capf_table **out);
/* join(other, joinType, (l, r)*) (Table.scala:99) */
capf_status capf_table_join(capf_table *l, capf_table *r, int32_t join_type, int32_t npairs,
                            const char *const *lcols, const char *const *rcols,
                            capf_table **out);
/* unionAll(other) (Table.scala:107) */
capf_status capf_table_union_all(capf_table *l, capf_table *r, capf_table **out);
/* orderBy((expr, order)*) (Table.scala:115) */
capf_status capf_table_order_by(capf_table *t, int32_t n, const capf_expr *keys,
                                const int32_t *descending, capf_table **out);
/* skip(n) / limit(n) (Table.scala:123, :131) */
capf_status capf_table_skip(capf_table *t, int64_t n, capf_table **out);
capf_status capf_table_limit(capf_table *t, int64_t n, capf_table **out);
/* distinct / distinct(cols*) (Table.scala:138, :146) */
capf_status capf_table_distinct(capf_table *t, capf_table **out);
capf_status capf_table_distinct_cols(capf_table *t, int32_t n, const char *const *cols,
                                     capf_table **out);
/* group(by, aggregations)(header, params) (Table.scala:158-159).
 * by_cols are the physical columns owned by the grouping vars
 * (header.ownedBy, FlinkTable.scala:129-135).                              */
capf_status capf_table_group(capf_table *t, int32_t n_by, const char *const *by_cols,
                             int32_t n_aggs, const int32_t *agg_kinds,
                             const capf_expr *agg_args, const int32_t *agg_distinct,
                             const char *const *agg_names, capf_table **out);
/* group with per-aggregator parameters: agg_params[i] is the percentile
 * fraction of CAPF_AGG_PERCENTILE_CONT / _DISC (ignored for the others; may
 * be NULL when no percentile is requested).  capf_table_group is this call
 * with agg_params = NULL.                                                  */
capf_status capf_table_group_ex(capf_table *t, int32_t n_by, const char *const *by_cols,
                                int32_t n_aggs, const int32_t *agg_kinds,
                                const capf_expr *agg_args, const int32_t *agg_distinct,
                                const double *agg_params, const char *const *agg_names,
                                capf_table **out);
/* withColumns((expr, col)*)(header, params) (Table.scala:170) */
capf_status capf_table_with_columns(capf_table *t, int32_t n, const capf_expr *exprs,
                                    const char *const *names, capf_table **out);
/* UNWIND: withColumns(Explode(list) AS item) (RelationalPlanner.scala:99-101,
 * Explode = FlinkSQLExprMapper.scala:101; row semantics of Spark's explode,
 * SparkSQLExprMapper.scala:146-149): every row of t is repeated once per
 * element of the list, the new column `name` holding the element (rows in
 * input order, elements in list order; an empty list drops the row).
 * capf_table_explode_values: the same literal / parameter list for every row:
 *   n elements of capf type `type` (INT64 / FLOAT64 / BOOL / STRING codes /
 *   NULL), values n × (8 or 1) bytes (NULL for a NULL-typed list), valid
 *   a NULL pointer (every element present) or n bytes (0 = a NULL element).
 * capf_table_explode_list: the elements of LIST column list_col (a NULL list
 *   drops the row, like an empty one; a NULL element is a row whose `name`
 *   is NULL).  Lazy like every other operator: t is
 *   evaluated with the result, unless list_col is a computed list expression
 *   (its element type is then only known once it exists).                  */
capf_status capf_table_explode_values(capf_table *t, const char *name, int32_t type, int64_t n,
                                      const void *values, const uint8_t *valid, capf_table **out);
capf_status capf_table_explode_list(capf_table *t, const char *list_col, const char *name,
                                    capf_table **out);
/* show(n) (Table.scala:177): prints to stdout */
capf_status capf_table_show(capf_table *t, int32_t rows);

/* ------------------------------------------------ synthetic graph inputs
 * Deterministic Graph500-style R-MAT generator (counter-based, identical to
 * oracle/rmat.c) writing straight into HBM.  Not part of the Table SPI:
 * it stands in for the graph-ingest step (EdgeListDataSource,
 * flink-cypher/.../api/io/edgelist/EdgeListDataSource.scala:56-92).
 * thresholds = floor(a*2^32), floor((a+b)*2^32), floor((a+b+c)*2^32).
 * Produces a relationship table with columns (id_col, src_col, dst_col),
 * rel ids = id_base + edge index, for edges [first, first+count).          */
capf_status capf_rmat_rel_table(capf_session *s, int32_t scale, uint64_t seed,
                                uint32_t t_a, uint32_t t_ab, uint32_t t_abc,
                                int64_t first, int64_t count, int64_t id_base,
                                const char *id_col, const char *src_col,
                                const char *dst_col, capf_table **out);
/* Node table with id column [base, base+n) and an optional BOOL label column
 * label_col (NULL = none) set with probability 1/2 from the seeded hash.  */
capf_status capf_range_node_table(capf_session *s, int64_t base, int64_t n, uint64_t seed,
                                  const char *id_col, const char *label_col,
                                  capf_table **out);

/* ------------------------------------------------------ edge-list ingest
 * EdgeListDataSource.graph (flink-cypher/.../api/io/edgelist/EdgeListDataSource.scala:61-81):
 * a CSV of two LONG fields per line (start, end), field delimiter `sep`
 * (option "sep"), lines beginning with `comment` (option "comment", may be
 * NULL) skipped — CsvTableSource.builder().field(.., LONG) ×2
 * .fieldDelimiter(sep).commentPrefix(comment) (:62-68).  Parsed on the GPU
 * into a relationship table (id_col, src_col, dst_col); ids are the data-line
 * ordinals 0..M-1, one valid zipWithUniqueId assignment (safeAddIdColumn,
 * flink-cypher/.../impl/TableOps.scala:217-238).  A malformed line fails the
 * call with CAPF_ERR_ILLEGAL_ARGUMENT naming the line (Flink: ParseException).
 * capf_edge_list_parse takes the file's bytes; capf_edge_list_read the path. */
capf_status capf_edge_list_parse(capf_session *s, const char *bytes, int64_t nbytes,
                                 const char *sep, const char *comment, const char *id_col,
                                 const char *src_col, const char *dst_col, capf_table **out);
capf_status capf_edge_list_read(capf_session *s, const char *path, const char *sep,
                                const char *comment, const char *id_col, const char *src_col,
                                const char *dst_col, capf_table **out);

/* ----------------------------------------- fused var-length reach (config 5)
 * The fused form of
 *   VarLengthExpand(a, [r*lower..upper], b)   VarLengthExpandPlanner.scala:82-259
 *   → Distinct(a, b)                          FlinkTable.scala:189-196
 *   → Aggregate(by a, count(*) AS reach)      FlinkTable.scala:123-150
 * over a directed relationship scan `rels` (src_col → dst_col), the source
 * node scan `sources` and the target node scan `targets`: one row
 * (out_source_col = a's id, out_reach_col = #distinct b) per source a that
 * reaches at least one target — the rows the relational plan produces,
 * without materialising the paths.  lower = 1 (rel isomorphism cannot change
 * the distinct pairs) and lower = 0 (the copyElement branch,
 * VarLengthExpandPlanner.scala:180-205: every source also pairs with itself,
 * so every source has a row; source ids unique) run the multi-source BFS.
 * 2 <= lower <= upper <= 4: from lower bound 2 the distinct pairs are those
 * joined by a TRAIL (pairwise distinct relationships), which one workgroup
 * per source enumerates; every row of `rels` is one relationship (parallel
 * rows are different relationships, a self-loop row is one), and the id
 * dictionary (rel endpoints, sources, targets) may hold at most 2^20 nodes.
 * Other bounds with lower >= 2, and a larger dictionary, return
 * CAPF_ERR_NOT_IMPLEMENTED and the caller plans the join chain.            */
capf_status capf_var_length_reach(capf_session *s, capf_table *rels, const char *src_col,
                                  const char *dst_col, capf_table *sources,
                                  const char *source_id_col, capf_table *targets,
                                  const char *target_id_col, int32_t lower, int32_t upper,
                                  const char *out_source_col, const char *out_reach_col,
                                  capf_table **out);
/* The same three operators over the UNDIRECTED pattern (a)-[r*lower..upper]-(b),
 * as UndirectedVarLengthExpandPlanner lowers it (VarLengthExpandPlanner.scala:277-307):
 * an automaton over states (node x, mode out | in) that starts at (a, out);
 * a relationship e not yet on the path leads
 *   (x, out), start(e) = x  ->  (end(e), out)
 *   (x, out), end(e) = x    ->  (start(e), in)
 *   (x, in),  start(e) = x  ->  (x, in)
 *   (x, in),  end(e) = x    ->  (x, out)
 * (after an inbound step the next step does not move), and every state reached
 * at depth max(lower, 1)..upper pairs a with its node when that node is a
 * target; lower = 0 adds (a, a) for every source.  Relationships on one path
 * are pairwise distinct rows of `rels` (parallel rows differ, a self-loop row
 * is one relationship, found from both of its node's sides).  This is neither
 * a walk nor a trail of the symmetrised graph, so every bound is answered by
 * per-source enumeration: 0 <= lower <= upper <= 4, at most 2^20 nodes in the
 * id dictionary.  Other bounds, and a larger dictionary, return
 * CAPF_ERR_NOT_IMPLEMENTED and the caller plans the join chain.            */
capf_status capf_var_length_reach_undirected(capf_session *s, capf_table *rels, const char *src_col,
                                             const char *dst_col, capf_table *sources,
                                             const char *source_id_col, capf_table *targets,
                                             const char *target_id_col, int32_t lower, int32_t upper,
                                             const char *out_source_col, const char *out_reach_col,
                                             capf_table **out);

/* ------------------------------------------------ multi-GPU partial counts
 * Building blocks of the hash-partitioned 2-hop count: the
 * caller (one process per GPU, torch.distributed/RCCL) exchanges the
 * per-node histograms between ranks.  See DESIGN.md "Multi-GPU".
 * capf_chain2_local_hists: over the rel rows of this rank, writes
 *   in_hist[mix(v - node_base)]  = #rels with dst = v   (v any node)
 *   out_hist[mix(v - node_base)] = #rels with src = v
 * for rels whose endpoints both lie in [node_base, node_base + n_nodes)
 * and returns the number of such self-loops.  Buffers are device uint32
 * arrays of capf_chain2_hist_len(n_nodes) = 2^k >= n_nodes entries, every
 * entry written by the call; mix is the bijection of 2^k node offsets
 * (odd multiply, xorshift; csrc/device_common.h node_mix) the radix
 * partitioning hashes by, so a contiguous 1/G slice of the histogram index
 * is a hash partition of the nodes.                                         */
/* Node-partitioned layout (SURVEY §8(e) "each rel is stored on owner(src);
 * for incoming expansion also a copy on owner(dst)"): owner(v) = the rank
 * whose contiguous range of 64 Ki-index buckets holds mix(v - node_base).
 * capf_table_node_partition: the rows of t whose key_col is owned by `part`
 * of `parts` (the out-copy with key = source, the in-copy with key = target).
 * capf_chain2_sharded_count: this rank's partial of the 2-hop count,
 *   Σ_{b owned} in[b]·out[b] − owned self-loops,
 * in[b] from the in-copy's target column, out[b] from the out-copy's source
 * column (its target column gives the self-loops).  Asynchronous on the
 * session stream; writes the int64 partial to device memory d_partial, ready
 * for one all-reduce (sum) over ranks.  Histograms are session scratch.      */
capf_status capf_table_node_partition(capf_table *t, const char *key_col, int64_t node_base,
                                      int64_t n_nodes, int32_t parts, int32_t part,
                                      capf_table **out);
capf_status capf_chain2_sharded_count(capf_session *s, capf_table *in_copy, const char *in_dst,
                                      capf_table *out_copy, const char *out_src,
                                      const char *out_dst, int64_t node_base, int64_t n_nodes,
                                      int32_t parts, int32_t part, int64_t *d_partial);
/* 2-D layout of the out-copy (a block partition of the adjacency matrix by
 * (owner(source), owner(target)), as distributed graph stores keep it):
 * capf_table_node_partition_diag returns the rows whose source `part` owns
 * with the rows whose target it owns too first (*n_diag of them);
 * capf_chain2_sharded_count_diag is capf_chain2_sharded_count for such an
 * out-copy: a self-loop has both endpoints owned, so the target column is
 * read for rows [0, n_diag) only (n_diag = -1: every row).  hot_ids: up to
 * 2 heavy-hitter node ids (host array; a plan hint sampled at ingest — any
 * ids give the same count): keys equal to one are counted in registers by
 * the partition pass instead of being partitioned (skew handling: a hub's
 * keys would pile onto one LDS counter word in the counting pass).          */
capf_status capf_table_node_partition_diag(capf_table *t, const char *src_col, const char *dst_col,
                                           int64_t node_base, int64_t n_nodes, int32_t parts,
                                           int32_t part, capf_table **out, int64_t *n_diag);
capf_status capf_chain2_sharded_count_diag(capf_session *s, capf_table *in_copy, const char *in_dst,
                                           capf_table *out_copy, const char *out_src,
                                           const char *out_dst, int64_t n_diag, int32_t n_hot,
                                           const int64_t *hot_ids, int64_t node_base,
                                           int64_t n_nodes, int32_t parts, int32_t part,
                                           int64_t *d_partial);
/* Directed triangle (a)-->(b)-->(c)-->(a) with pairwise distinct rels over
 * the rels of `rels` whose endpoints lie in [node_base, node_base + n_nodes)
 * (the fused form of Expand, Expand, ExpandInto + uniqueness,
 * RelationalPlanner.scala:130-189): part `part` of `parts` of the count as a
 * device int64 at d_count — the parts sum to the count (rank r of G computes
 * part r over a replicated rel table, then one all-reduce).  Asynchronous on
 * the session stream after two internal host reads.                         */
capf_status capf_triangle_count_part(capf_session *s, capf_table *rels, const char *src_col,
                                     const char *dst_col, int64_t node_base, int64_t n_nodes,
                                     int32_t parts, int32_t part, int64_t *d_count);
int64_t capf_chain2_hist_len(int64_t n_nodes);
capf_status capf_chain2_local_hists(capf_session *s, capf_table *rels, const char *src_col,
                                    const char *dst_col, int64_t node_base, int64_t n_nodes,
                                    uint32_t *d_in_hist, uint32_t *d_out_hist,
                                    int64_t *self_loops);
/* Diagnostics, host only (no device is touched): the length in tiles of the
 * job that a unit of the indexed 2-hop count claims from an out-run of `ntiles`
 * tiles holding `run_pieces` pieces, when it last saw the run's cursor at tile
 * `pos`.  mean_pieces: a mean run's pieces; job_split: the jobs a mean run is cut
 * into (CAPF_C5_JOB_SPLIT); excess_split: crumbs to the weight of one such job
 * for the part of a run above the mean (CAPF_C5_EXCESS_SPLIT, 0: one length per
 * run); min_tiles: the shortest job (CAPF_C5_STEAL_TILES).                  */
uint32_t capf_c5_job_len(uint32_t run_pieces, uint32_t mean_pieces, uint32_t job_split,
                         uint32_t excess_split, uint32_t ntiles, uint32_t min_tiles, uint32_t pos);
/* Σ_v a[v]·b[v] over n entries (device uint32 arrays), exact in uint64. */
capf_status capf_dot_u32(capf_session *s, const uint32_t *d_a, const uint32_t *d_b, int64_t n,
                         uint64_t *out);

/* CSV tables of an FS graph source whose declared fields are all LONG
 * (FSGraphSource.readFromCsv, flink-cypher/.../api/io/fs/FSGraphSource.scala:80-84:
 * Flink's CsvTableSource over the canonical field list of CAPFGraphExport —
 * id, source, target and INTEGER properties).  One INT64 column per declared
 * field, in file order; row rules as capf_edge_list_read (LongParser, trailing
 * '\r' stripped, short rows / empty fields / overflow fail the read naming the
 * line); text after the last declared field is not read.  ncols ≤ 16.      */
capf_status capf_csv_parse_longs(capf_session *s, const char *bytes, int64_t nbytes,
                                 const char *sep, int32_t ncols, const char *const *names,
                                 capf_table **out);
capf_status capf_csv_read_longs(capf_session *s, const char *path, const char *sep,
                                int32_t ncols, const char *const *names, capf_table **out);

/* CSV tables of an FS graph source with typed fields, parsed on the GPU: one
 * column per declared field, in file order, of type types[i] — CAPF_TYPE_INT64,
 * FLOAT64, BOOL, STRING, DATE or LOCALDATETIME (anything else is
 * IllegalArgument).  ncols ≤ 16; sep is 1 to 8 ASCII bytes; text after the last
 * declared field is not parsed.  Lines as Python's text mode reads them: '\n'
 * ends a line, one '\r' directly before it (or at the end of the file) is
 * stripped, any other '\r' rejects the file, as does a line with fewer fields
 * than declared.  An empty field is NULL for every type; a column without a
 * NULL carries no validity mask.  Fields:
 *   INT64          optional '-' and ASCII digits within int64 (as _longs)
 *   BOOL           true | false, ASCII case-insensitive
 *   DATE           YYYY-MM-DD, year 0001-9999, a day of the Gregorian month
 *   LOCALDATETIME  YYYY-MM-DDTHH:MM:SS[.f{1,6}], hour ≤ 23, minute, second ≤ 59
 *   FLOAT64        [+-]?(\d+(\.\d*)?|\.\d+)([eE][+-]?\d+)?, correctly rounded
 *                  (the device converts mantissas ≤ 2^53 with |power of ten|
 *                  ≤ 22 exactly; the others are converted on the host after the
 *                  kernel — capf_session_csv_slow_floats counts them)
 *   STRING         the field's bytes, interned on the device: strict UTF-8
 *                  without 0x00
 * A byte ≥ 0x80 outside a STRING field (the unparsed text included) rejects
 * the file.  A rejection is IllegalArgument, "CSV line N could not be parsed:
 * <reason>", N the first bad line (1-based).  No quoting, no comment prefix. */
capf_status capf_csv_parse_typed(capf_session *s, const char *bytes, int64_t nbytes, const char *sep,
                                 int32_t ncols, const char *const *names, const int32_t *types,
                                 capf_table **out);
capf_status capf_csv_read_typed(capf_session *s, const char *path, const char *sep,
                                int32_t ncols, const char *const *names, const int32_t *types,
                                capf_table **out);
/* FLOAT64 fields that the session's last capf_csv_*_typed call converted on the host. */
capf_status capf_session_csv_slow_floats(capf_session *s, int64_t *out);

/* ------------------------------------------------- distributed Table layer
 * The exchange of a hash-partitioned Table over G ranks (dist_table.py):
 * Flink's join and groupBy repartition both inputs by a hash of the key
 * before the local operator (FlinkTable.scala:171-187 join, :123-150 group
 * lower onto DataSet joinWithTiny/hash-partitioned join and groupBy); here
 * the repartition is this call plus one all-to-all per column (RCCL).
 * capf_table_hash_route: a materialised copy of t whose rows are grouped by
 *   owner = h(values of keys[0..nkeys)) of `parts` (owner order, stable inside
 *   an owner); counts[p] = rows owned by p (host array of `parts`).  Equal key
 *   tuples have equal owners; NULLs of a key route together; −0.0 as 0.0.
 *   LIST columns are carried along with their rows; a LIST column as a
 *   routing key is refused (CAPF_ERR_ILLEGAL_ARGUMENT).
 * capf_table_download_device: `rows` of one column into DEVICE buffers
 *   (decoded values, size × 8 or 1 bytes; d_valid = size bytes, 1 = present).
 * capf_table_has_nulls: does column col carry a validity array (or is it
 *   an all-NULL column with rows)?                                          */
capf_status capf_table_hash_route(capf_table *t, int32_t nkeys, const char *const *keys,
                                  int32_t parts, int64_t *counts, capf_table **out);
capf_status capf_table_download_device(capf_table *t, const char *col, void *d_values,
                                       uint8_t *d_valid);
capf_status capf_table_has_nulls(capf_table *t, const char *col, int32_t *has);

/* Exchange wire format of the distributed Table layer (dist_table.py: one
 * all_to_all_single per shuffle, Flink's hash repartition in FlinkTable.scala:
 * 123-196).  A row is packed as, per column i: width[i] bytes of
 * (value − base[i]) little-endian — 3 / 4 for INTEGER / STRING columns whose
 * range over every rank fits 24 / 32 bits (FOR24 / FOR32), 8 otherwise and for
 * FLOAT (base 0), 1 for BOOL, 0 for NULL — then one validity byte when
 * nullable[i].  capf_table_column_range: min / max / non-NULL count of an
 * INTEGER or STRING column (column statistics, computed once).
 * capf_table_pack_rows: *row_bytes = W; rows into d_out (n·W device bytes; null
 * d_out: only W).  capf_table_from_packed_rows: the table of nrows packed rows
 * at d_rows (copied out; the narrow widths stay FOR24 / FOR32 encoded).
 * DATE and LOCALDATETIME columns are packed like INTEGER columns.
 *
 * LIST columns.  Row part: a LIST column contributes a length field to the
 * packed row — the list's element count little-endian, 0 for a NULL list —
 * width[i] = 4 when the longest list over all ranks has fewer than 2^31
 * elements, else 8 (base 0); then the usual validity byte when nullable[i].
 * Element stream: the elements travel beside the rows as the packed rows of
 * the child column taken as a one-column table, i.e. the record above for a
 * scalar column of the element type: `width` bytes of (value − base) — 3 / 4
 * for INTEGER and STRING-code elements whose range over all ranks fits 24 /
 * 32 bits, 8 otherwise and for FLOAT, 1 for BOOLEAN, 0 for NULL-typed
 * elements (only the lengths travel; the receiver rebuilds a NULL child of
 * the summed length) — then one validity byte when an element is NULL on some
 * rank.  The rows for rank p are a contiguous slice of the routed table, so
 * its elements are the contiguous slice [off[r_p], off[r_p + counts[p]]) of
 * the stream: the element send counts are differences of offsets.
 * capf_table_pack_rows accepts LIST columns (width 4 or 8);
 * capf_table_from_packed_rows does not (use capf_table_from_packed_lists).
 * capf_table_list_stats: what the layout agreement needs of a LIST column:
 *   element type, longest (non-NULL) list, element count, whether an element
 *   is NULL, the element column's physical encoding (0 plain, 1 FOR32,
 *   2 FOR24), and min / max / non-NULL count of INTEGER / STRING-code elements
 *   (max < min: none).
 * capf_table_pack_list_elems: the element stream of LIST column col for rows
 *   split into nparts consecutive slices of row_counts[p] rows (they must sum
 *   to the table's rows): elem_counts[p] = elements of slice p, *rec_bytes =
 *   width + (elem_nullable ? 1 : 0), the records into d_out (Σ elem_counts ·
 *   rec_bytes device bytes, 4-byte aligned, 8-byte for 8-byte records; null
 *   d_out: sizes only).  A NULL list is empty on the wire: where a NULL list
 *   owns elements in the column (capf_table_add_list accepts offsets that
 *   give it some), they are left out of the stream and of the counts, here
 *   and in capf_table_list_stats, so the receiver's NULL lists own none.  elem_type
 *   is the agreed element type: the column's own, or any type when the
 *   column's elements are NULL-typed (they are then sent as NULL elements of
 *   that type and need the validity byte).
 * capf_table_from_packed_lists: capf_table_from_packed_rows for rows with LIST
 *   columns: the l-th LIST column (in column order) takes element stream l —
 *   n_elems[l] records at d_elems[l] (4-byte aligned) of elem_width[l] bytes
 *   (+ validity byte when elem_nullable[l]) of type elem_types[l].  The rows'
 *   lengths must sum to n_elems[l].  The child keeps the narrow encoding.
 * Bad arguments (counts that do not sum to the rows, a width that does not fit
 * the element type, NULL elements without their validity byte, a LIST column
 * named where a scalar is expected or the reverse) are
 * CAPF_ERR_ILLEGAL_ARGUMENT.                                                  */
capf_status capf_table_column_range(capf_table *t, const char *col, int64_t *min, int64_t *max,
                                    int64_t *non_null);
capf_status capf_table_pack_rows(capf_table *t, int32_t ncols, const char *const *cols, const int32_t *width,
                                 const int64_t *base, const int32_t *nullable, int32_t *row_bytes, void *d_out);
capf_status capf_table_from_packed_rows(capf_session *s, int32_t ncols, const char *const *names,
                                        const int32_t *types, const int32_t *width, const int64_t *base,
                                        const int32_t *nullable, const void *d_rows, int64_t nrows,
                                        capf_table **out);
capf_status capf_table_list_stats(capf_table *t, const char *col, int32_t *elem_type, int64_t *longest,
                                  int64_t *n_elems, int32_t *elem_nulls, int32_t *elem_enc, int64_t *min,
                                  int64_t *max, int64_t *non_null);
capf_status capf_table_pack_list_elems(capf_table *t, const char *col, int32_t nparts, const int64_t *row_counts,
                                       int32_t elem_type, int32_t width, int64_t base, int32_t elem_nullable,
                                       int64_t *elem_counts, int32_t *rec_bytes, void *d_out);
capf_status capf_table_from_packed_lists(capf_session *s, int32_t ncols, const char *const *names,
                                         const int32_t *types, const int32_t *width, const int64_t *base,
                                         const int32_t *nullable, const void *d_rows, int64_t nrows, int32_t nlists,
                                         const int32_t *elem_types, const int32_t *elem_width,
                                         const int64_t *elem_base, const int32_t *elem_nullable,
                                         const void *const *d_elems, const int64_t *n_elems, capf_table **out);

/* ------------------------------------------------- rank communicator (RCCL)
 * The exchange of the distributed Table layer for hosts without a framework
 * communicator (the JVM twin DistGpuTable.scala; the Python layer uses
 * torch.distributed for the same collectives): RCCL over xGMI, one process per
 * GPU, every collective enqueued on the session's stream (ordered with the
 * kernels that produce and consume its buffers).  It replaces Flink's hash
 * repartition between operator instances (FlinkTable.scala:123-196).
 * capf_comm_unique_id: rank 0 creates the id (128 bytes) and sends it to the
 *   other ranks out of band; every rank then calls capf_comm_init with it.
 * capf_comm_all_reduce_i64: in place, op CAPF_COMM_SUM / CAPF_COMM_MAX.
 * capf_comm_all_gather_bytes: `bytes` from every rank, rank-major into d_recv
 *   (world × bytes).
 * capf_comm_all_to_all_bytes: send_bytes[p] bytes (consecutive in d_send, rank
 *   order) to rank p, recv_bytes[p] from rank p into d_recv (rank order) —
 *   the packed-row shuffle of capf_table_pack_rows.
 * capf_session_alloc / capf_session_free: device buffers from the session's
 *   stream-ordered pool (exchange buffers, count slots);
 * capf_session_copy: hipMemcpyAsync on the session stream + wait (kind 1 =
 *   host → device, 2 = device → host, 3 = device → device).               */
#define CAPF_COMM_ID_BYTES 128
enum { CAPF_COMM_SUM = 0, CAPF_COMM_MAX = 2 };
typedef struct capf_comm capf_comm;
capf_status capf_comm_unique_id(uint8_t *id_out);
capf_status capf_comm_init(capf_session *s, int32_t world, int32_t rank, const uint8_t *id, capf_comm **out);
capf_status capf_comm_destroy(capf_comm *c);
capf_status capf_comm_rank(capf_comm *c, int32_t *rank, int32_t *world);
capf_status capf_comm_all_reduce_i64(capf_comm *c, int64_t *d_buf, int64_t n, int32_t op);
capf_status capf_comm_all_gather_bytes(capf_comm *c, const void *d_send, int64_t bytes, void *d_recv);
capf_status capf_comm_all_to_all_bytes(capf_comm *c, const void *d_send, const int64_t *send_bytes,
                                       void *d_recv, const int64_t *recv_bytes);
capf_status capf_session_alloc(capf_session *s, int64_t bytes, void **d_out);
capf_status capf_session_free(capf_session *s, void *d);
capf_status capf_session_copy(capf_session *s, void *dst, const void *src, int64_t bytes, int32_t kind);

/* A literal set for CAPF_OP_IN_SET: the n int64 values (INTEGER values or
 * STRING dictionary codes) sorted and deduplicated into device memory owned by
 * the session; *set_id names it in programs as "\x01set:<set_id>".  The same
 * values registered again return the same id. */
capf_status capf_session_literal_set(capf_session *s, const int64_t *values, int64_t n, int32_t *set_id);
/* A code map of CAPF_OP_STR_MAP: codes[c] = the STRING code the function gives
 * dictionary string c (−1: NULL), for c < n.  The caller (the shim) applies the
 * function on the host with the JVM's string semantics and interns the
 * results; the map is referenced in programs as "\x01map:<id>" (*map_id).  */
capf_status capf_session_code_map(capf_session *s, const int64_t *codes, int64_t n, int32_t *map_id);
/* The code map map_id grown to n entries after the dictionary has grown:
 * codes[0 .. old n) must be the map's codes.  Replaced in place (*new_id =
 * map_id; the old table is released once the launches already enqueued have
 * read it, and programs naming the id read the longer map) when this is the
 * map's only registration; otherwise (equal maps registered for several
 * functions) a new map is registered and *new_id names it.               */
capf_status capf_session_code_map_extend(capf_session *s, int32_t map_id, const int64_t *codes, int64_t n,
                                         int32_t *new_id);
/* A LIST property column from host data (CTList properties of element tables,
 * CAPFElementTable.create / FlinkConversions.scala:43-117 map CTList to an
 * ARRAY column): appends LIST column `name` to t's rows (t is materialised):
 * row i holds values[offsets[i] .. offsets[i + 1]) (offsets: size + 1 int64,
 * offsets[0] = 0), elements of capf type elem_type (INTEGER / FLOAT / BOOLEAN
 * / STRING codes, 8 B each, BOOLEAN 1 B; every element present); valid (size
 * bytes or NULL): 0 = a NULL list.
 * capf_table_add_list_nulls: the same with element validity elem_valid
 * (offsets[size] bytes, 0 = a NULL element, or NULL: every element present).
 * elem_type may be CAPF_TYPE_NULL with values NULL: every element is NULL.  */
capf_status capf_table_add_list(capf_table *t, const char *name, int32_t elem_type, const int64_t *offsets,
                                const void *values, const uint8_t *valid, capf_table **out);
capf_status capf_table_add_list_nulls(capf_table *t, const char *name, int32_t elem_type, const int64_t *offsets,
                                      const void *values, const uint8_t *valid, const uint8_t *elem_valid,
                                      capf_table **out);

/* This table plus LIST column `name` whose row i holds (cols[0][i], ...,
 * cols[n-1][i]) — a list literal of per-row elements, `[n.val * 10, $p]`
 * (replaces FlinkSQLExprMapper.scala:71 `array(...)` over the converted
 * children).  The non-NULL-typed element columns share one type (INTEGER and
 * FLOAT widen to FLOAT), the list's element type; CAPF_TYPE_NULL when every
 * item is NULL-typed.  A NULL item value is a NULL element (the element
 * column then carries validity; without nullable items it carries none).
 * Nested lists are NotImplemented.  n = 0: the empty list.                  */
capf_status capf_table_list_columns(capf_table *t, int32_t n, const char *const *cols, const char *name,
                                    capf_table **out);
/* List functions (okapi Expr.scala:640-653 Head / Last / Reverse, :859-880
 * Range, :1166-1176 ListSliceFromTo / ListSliceFrom / ListSliceTo, Add on
 * lists; Flink's mapper lowers none of them — the semantics are the Morpheus
 * lowering, SparkSQLExprMapper.scala:171-182, 265, 269, 336-338 and
 * MorpheusFunctions.scala:79-83, with Cypher's answers for negative and
 * crossing slice bounds; expectations FunctionTests.scala:1502-1556,
 * 1631-1718, ExpressionTests.scala:47-80, NullTests.scala:55-63, 107).
 * This table plus LIST column `name` = fn(args); args are column names of t,
 * an empty name an absent slice bound / step:
 *   SLICE   (list, from, to): Python's xs[from:to] — negative bounds count
 *           from the end, bounds are clamped, from >= to is the empty list;
 *           an EMPTY list gives NULL (ExpressionTests.scala:70-79), so does a
 *           NULL list or a NULL bound.  Bounds are INTEGER.
 *   REVERSE (list): the elements in reverse order, NULL elements included.
 *   CONCAT  (a, b): each a LIST or a scalar column; a scalar side is a
 *           one-element list (a NULL value a NULL element), a NULL list side
 *           gives NULL.  Element types are equal, or INTEGER with FLOAT
 *           (widened to FLOAT); a NULL-typed side takes the other's type;
 *           other mixes are NotImplemented ("Lists of different inner types
 *           are not supported", SparkSQLExprMapper.scala:179).
 *   RANGE   (from, to, step): INTEGER columns, step 1 when absent, the end
 *           inclusive; a direction that never arrives is the empty list, a
 *           NULL argument a NULL list.  A step of 0, or a row of more than
 *           2^31 - 1 elements (Spark's sequence limit), is IllegalArgument,
 *           raised when the table is evaluated.  No length or element wraps.
 * The node is lazy; its element type is known when it is built.
 * A NULL-typed list argument of SLICE / REVERSE gives a NULL-typed column. */
enum { CAPF_LIST_FN_SLICE = 0, CAPF_LIST_FN_REVERSE = 1, CAPF_LIST_FN_CONCAT = 2, CAPF_LIST_FN_RANGE = 3 };
capf_status capf_table_list_fn(capf_table *t, int32_t fn, int32_t nargs, const char *const *args,
                               const char *name, capf_table **out);
/* Lambda expressions over a list (okapi Expr.scala:199 LambdaVar, :1178-1237
 * ListComprehension / ListReduction / ListFilter / ListAny / ListNone /
 * ListAll / ListSingle; Flink's mapper lowers none of them — the semantics are
 * the Morpheus lowering, SparkSQLExprMapper.scala:340-395, on Spark 2.4.3
 * (build.params.gradle:21): filter / transform / exists / aggregate;
 * expectations ExpressionTests.scala:1502-1560, 1575-1643).  This table plus
 * column `name`.  `list` is a LIST column of t; `pred` and `body` are programs
 * over t's columns that may hold CAPF_OP_LAMBDA; they run once per list
 * ELEMENT, columns and list opcodes read at the row that owns the element.
 * #T = the number of the row's elements whose `pred` is TRUE (a NULL result
 * is not TRUE: Spark 2.4's filter and exists treat it as false):
 *   COMPREHENSION [x IN xs WHERE pred | body]: the elements with pred TRUE, in
 *           order, each mapped through body.  pred NULL: every element.  body
 *           NULL: the element itself (filter(x IN xs WHERE pred)).  A NULL
 *           element is bound as NULL.  A NULL list gives NULL, an empty list
 *           [].  out_type = the element type of the result (body's type, else
 *           the list's element type); element validity exists only when body
 *           (or the source element) can be NULL.
 *   ANY     #T > 0 (empty: FALSE)        NONE    #T = 0 (empty: TRUE)
 *   ALL     #T = size(xs) (empty: TRUE; a NULL pred result makes it FALSE)
 *   SINGLE  #T = 1
 *           A NULL list gives NULL for all four: ALL and SINGLE compare
 *           size(xs), which is NULL here (CAPF_OP_LIST_SIZE), not Spark's -1.
 *   REDUCE  reduce(acc = init, x IN xs | body): a left fold in list order,
 *           slot 0 the accumulator, slot 1 the element; `init` is a column of
 *           t.  A NULL list gives NULL, an empty list init.  NULLs flow
 *           through body by the interpreter's rules; INTEGER arithmetic wraps
 *           as CAPF_OP_ADD.  out_type = the result type: init's type when body
 *           (with the accumulator typed so) gives it; FLOAT for an INTEGER
 *           init with a FLOAT body (init widened); body's for a NULL-typed
 *           init; any other mix is IllegalArgument (Expr.scala:1196-1199).
 * The node is lazy and type-checked when built: `list` must be a LIST or
 * NULL-typed column (a NULL-typed one gives a NULL-typed column), a
 * quantifier needs `pred`, REDUCE needs `body` and `init` (else `init` is "").
 * Nested lists are NotImplemented.                                           */
enum { CAPF_LAMBDA_COMPREHENSION = 0, CAPF_LAMBDA_ANY = 1, CAPF_LAMBDA_ALL = 2,
       CAPF_LAMBDA_NONE = 3, CAPF_LAMBDA_SINGLE = 4, CAPF_LAMBDA_REDUCE = 5 };
capf_status capf_table_list_lambda(capf_table *t, int32_t kind, const char *list,
                                   const capf_expr *pred,  /* NULL: no WHERE            */
                                   const capf_expr *body,  /* NULL: no extract / n.a.   */
                                   const char *init,       /* REDUCE: column name, else "" */
                                   int32_t out_type,       /* element / result capf type */
                                   const char *name, capf_table **out);
/* split(original, delimiter) (okapi Split, Expr.scala:904-912; the Morpheus
 * lowering StringSplit, SparkSQLExprMapper.scala:272; expectations
 * FunctionTests.scala:1721-1746): this table plus LIST<STRING> column `name`,
 * row i = the pieces of str_col[i] between the leftmost non-overlapping
 * occurrences of delim_col[i], compared byte for byte on the device string
 * heap: matches + 1 pieces, trailing and inner empty strings kept, a subject
 * without a match one piece (itself; "" gives [""]).  That is what
 * java.lang.String.split(regex, -1) computes for a delimiter that is non-empty
 * and holds no regex metacharacter; the caller evaluates every other
 * delimiter itself.  A NULL operand gives a NULL list; elements are never
 * NULL.  The pieces are interned on the device (new codes ascend by the
 * smallest piece position producing each string).
 * The node is lazy and type-checked when built: both columns are STRING or
 * NULL-typed (a NULL-typed one gives a NULL-typed column), anything else is
 * IllegalArgument.  A row whose delimiter is the empty string is
 * IllegalArgument, raised when the table is evaluated.                      */
capf_status capf_table_str_split(capf_table *t, const char *str_col, const char *delim_col,
                                 const char *name, capf_table **out);
/* labels(n) / keys(n) (FlinkSQLExprMapper.scala:136-153; the GetLabels /
 * GetKeys UDFs, :310-329): appends LIST<STRING> column `name` holding, per row,
 * codes[j] for each column cols[j] that holds TRUE (kinds[j] = 0, a label flag)
 * or any value (kinds[j] = 1, a property), in the given order (the shim sorts
 * by label / key name); never NULL (an empty list).                        */
capf_status capf_table_name_list(capf_table *t, int32_t n, const char *const *cols, const int32_t *kinds,
                                 const int64_t *codes, const char *name, capf_table **out);
/* A value map of CAPF_OP_VALUE_MAP: n keys (keys2 = NULL) or key pairs sorted
 * ascending as signed int64 (pairs lexicographically), codes[i] the STRING code
 * of entry i; referenced as "\x01vmap:<id>" (*map_id).                      */
capf_status capf_session_value_map(capf_session *s, const int64_t *keys, const int64_t *keys2, const int64_t *codes,
                                   int64_t n, int32_t *map_id);

/* String functions with literal arguments (FlinkSQLExprMapper.scala:187-195)
 * evaluated on the session's device string heap, the results interned on the
 * device.  iarg0 / iarg1: SUBSTRING's 1-based `from` and `len` (UTF-16 units,
 * Calcite's SUBSTRING; len >= 0).  lit0: the literal of CONCAT_L (literal + s)
 * / CONCAT_R (s + literal), or REPLACE's search literal (non-empty, matched
 * byte for byte, leftmost and non-overlapping); lit1: REPLACE's replacement —
 * dictionary codes.  Unused arguments are ignored.                          */
enum {
  CAPF_STR_FN_UPPER = 0,
  CAPF_STR_FN_LOWER = 1,
  CAPF_STR_FN_TRIM = 2,   /* TRIM / LTRIM / RTRIM strip ' ' (0x20) only */
  CAPF_STR_FN_LTRIM = 3,
  CAPF_STR_FN_RTRIM = 4,
  CAPF_STR_FN_SUBSTRING = 5,
  CAPF_STR_FN_CONCAT_L = 6,
  CAPF_STR_FN_CONCAT_R = 7,
  CAPF_STR_FN_REPLACE = 8
};
/* out[i] (host, n entries) = the code of fn applied to dictionary string
 * src[i] — or, src NULL, to string c0 + i (a range of the dictionary); −1 where
 * src[i] is −1 (NULL); −2 where the caller must evaluate the function itself
 * with the JVM's semantics: UPPER / LOWER of a string with a byte >= 0x80,
 * SUBSTRING of a string with a supplementary character, REPLACE in a subject
 * of at least CAPF_STR_LONG bytes.  Results new to the dictionary are appended
 * to it with ascending codes in the order of the first i producing each, so
 * equal dictionaries given equal calls stay equal.  IllegalArgument: an
 * unknown fn, a code out of range, len < 0, an empty search literal.        */
capf_status capf_string_fn_codes(capf_session *s, int32_t fn, int64_t iarg0, int64_t iarg1, int64_t lit0,
                                 int64_t lit1, const int64_t *src, int64_t c0, int64_t n, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* CAPF_GPU_H */
