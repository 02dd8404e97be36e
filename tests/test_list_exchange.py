"""LIST columns on the exchange wire (csrc/shuffle.hip "list elements",
include/capf_gpu.h "LIST columns"): route → pack rows → pack elements → build
from packed, through the C-ABI at world size one and over routed
destinations; the argument errors; the JNI / Scala declarations; and the
width selection of dist_table.py (a pure helper, no GPU)."""
import os
import re
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_NULL, T_INT, T_FLOAT, T_BOOL, T_STRING, T_LIST = 0, 1, 2, 3, 4, 5
ENC_PLAIN, ENC_FOR32, ENC_FOR24 = 0, 1, 2
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

gpu = pytest.mark.gpu


# ------------------------------------------------------------ C-ABI helpers
def _list_stats(t, col):
    from capf_amd import _lib
    et, en, enc = c_int32(), c_int32(), c_int32()
    longest, ne, mn, mx, nn = c_int64(), c_int64(), c_int64(), c_int64(), c_int64()
    _lib.call("capf_table_list_stats", t._h, col.encode(), byref(et), byref(longest), byref(ne), byref(en),
              byref(enc), byref(mn), byref(mx), byref(nn))
    return dict(et=et.value, longest=longest.value, n_elems=ne.value, nulls=bool(en.value), enc=enc.value,
                min=mn.value, max=mx.value, non_null=nn.value)


def _layout(t, key="k", col="xs"):
    """The layout dist_table.py's _layout picks at world size one: (row widths,
    bases, nullables) for (key, col) and the element (type, width, base, nullable)."""
    from capf_amd import _lib
    from capf_amd.dist_table import length_width, range_entries, scalar_wire
    st = _list_stats(t, col)
    neg_min, mx = range_entries(st["min"], st["max"], st["non_null"])  # what the MAX all-reduce would carry
    ew, eb = scalar_wire(st["et"], -neg_min, mx)
    has = c_int32()
    _lib.call("capf_table_has_nulls", t._h, col.encode(), byref(has))
    rows = ([8, length_width(st["longest"])], [0, 0], [0, int(bool(has.value))])
    return rows, (st["et"], ew, eb, int(st["nulls"] and st["et"] != T_NULL))


def _route(s, t, keys, parts):
    from capf_amd import _lib
    from capf_amd.table import GpuTable
    counts = (c_int64 * parts)()
    h = c_void_p()
    _lib.call("capf_table_hash_route", t._h, len(keys), _lib.strs(keys), parts, counts, byref(h))
    return GpuTable(s, h), list(counts)


def _pack(t, counts, rows, elem, key="k", col="xs"):
    """(packed rows uint8 [n, W], element records uint8 [total, rec], element counts per slice)."""
    import torch
    from capf_amd import _lib
    width, base, nullable = rows
    cols = [key, col]
    arrs = (_lib.strs(cols), (c_int32 * 2)(*width), (c_int64 * 2)(*base), (c_int32 * 2)(*nullable))
    W = c_int32()
    _lib.call("capf_table_pack_rows", t._h, 2, *arrs, byref(W), None)
    assert W.value == sum(width) + sum(nullable)
    n = t.size
    d_rows = torch.zeros(max(n * W.value, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the fill ran on torch's stream, the packer runs on the session's
    _lib.call("capf_table_pack_rows", t._h, 2, *arrs, byref(W), c_void_p(d_rows.data_ptr()))
    et, ew, eb, en = elem
    rc = (c_int64 * len(counts))(*counts)
    ec = (c_int64 * len(counts))()
    rec = c_int32()
    args = (t._h, col.encode(), len(counts), rc, et, ew, eb, en, ec, byref(rec))
    _lib.call("capf_table_pack_list_elems", *args, None)  # sizes only
    assert rec.value == ew + en
    total = sum(ec)
    # a canary past the records: the packer writes total · rec bytes and not one more
    d_el = torch.full((total * rec.value + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.call("capf_table_pack_list_elems", *args, c_void_p(d_el.data_ptr()))
    assert (d_el[total * rec.value:] == 0xA5).all()
    return (d_rows[:n * W.value].view(n, W.value), d_el[:total * rec.value].view(total, rec.value), list(ec))


def _unpack(s, d_rows, d_el, rows, elem, key="k", col="xs"):
    from capf_amd import _lib
    from capf_amd.table import GpuTable
    width, base, nullable = rows
    et, ew, eb, en = elem
    m, ne = d_rows.shape[0], d_el.shape[0]
    import torch
    d_rows, d_el = d_rows.contiguous().clone(), d_el.contiguous().clone()  # fresh (aligned) buffers
    torch.cuda.synchronize()  # the copies ran on torch's stream
    h = c_void_p()
    _lib.call("capf_table_from_packed_lists", s._h, 2, _lib.strs([key, col]), (c_int32 * 2)(T_INT, T_LIST),
              (c_int32 * 2)(*width), (c_int64 * 2)(*base), (c_int32 * 2)(*nullable),
              c_void_p(d_rows.data_ptr() if d_rows.numel() else 0), m, 1, (c_int32 * 1)(et), (c_int32 * 1)(ew),
              (c_int64 * 1)(eb), (c_int32 * 1)(en), (c_void_p * 1)(d_el.data_ptr() if d_el.numel() else 0),
              (c_int64 * 1)(ne), byref(h))
    return GpuTable(s, h)


def _round_trip(s, t):
    routed, counts = _route(s, t, ["k"], 1)
    assert counts == [t.size]
    rows, elem = _layout(routed)
    d_rows, d_el, ec = _pack(routed, counts, rows, elem)
    assert ec == [_list_stats(routed, "xs")["n_elems"]]
    return _unpack(s, d_rows, d_el, rows, elem), elem


def _list_bag(t):
    """Multiset of (key, list) with elements by exact bit pattern (floats) and
    validity: ((key, None | tuple of None | int bits), …) sorted."""
    keys = t.column_arrays("k")[0].tolist()
    et, offs, vals, valid, ev = t.list_arrays("xs")
    bits = vals.view(np.int64) if et == T_FLOAT else vals.astype(np.int64)
    bits = np.where(ev.astype(bool), bits, 0) if ev is not None else bits
    ok = ev.astype(bool) if ev is not None else np.ones(len(bits), bool)
    if et == T_NULL:
        ok = np.zeros(len(bits), bool)
    out = []
    for i, k in enumerate(keys):
        if not valid[i]:
            out.append((k, None))
        else:
            a, b = offs[i], offs[i + 1]
            out.append((k, tuple(x if o else None for x, o in zip(bits[a:b].tolist(), ok[a:b].tolist()))))
    return sorted(out, key=repr)


def _random_lists(rng, n, draw, null_elems=True, mean=4):
    """n lists: ~1/8 NULL lists, ~1/8 empty, NULL elements sprinkled in."""
    out = []
    for i in range(n):
        u = rng.random()
        if u < 0.125:
            out.append(None)
        elif u < 0.25:
            out.append([])
        else:
            xs = [draw() for _ in range(int(rng.integers(1, 2 * mean)))]
            if null_elems and rng.random() < 0.3:
                xs[int(rng.integers(0, len(xs)))] = None
            out.append(xs)
    out[0], out[1], out[2] = None, [], [draw(), None]  # each kind at least once
    return out


N = 1003  # not a multiple of 4 or of the block

ELEM_CASES = {
    # name: (draw(rng) → element, expected element type, width, receiver's child encoding)
    "int24": (lambda r: int(r.integers(-5_000_000, 5_000_000)), T_INT, 3, ENC_FOR24),
    "int32": (lambda r: int(r.integers(-(1 << 31) + 5, (1 << 31) - 5)), T_INT, 4, ENC_FOR32),
    "int64_edges": (lambda r: [INT64_MIN, INT64_MAX, 0, -1, 1 << 40][int(r.integers(0, 5))], T_INT, 8, ENC_PLAIN),
    "float": (lambda r: [float("nan"), -0.0, 0.0, float("inf"), float("-inf"), 1.5, -2.25e300][int(r.integers(0, 7))],
              T_FLOAT, 8, ENC_PLAIN),
    "bool": (lambda r: bool(r.integers(0, 2)), T_BOOL, 1, ENC_PLAIN),
    "string": (lambda r: "s%d" % int(r.integers(0, 50)), T_STRING, 3, ENC_FOR24),
}


@gpu
@pytest.mark.parametrize("name", list(ELEM_CASES))
def test_round_trip_per_element_type(gpu_session, name):
    """1,003 rows with NULL lists, empty lists and NULL elements: the table
    built from the packed rows and element records holds the uploaded
    (key, list) multiset, and the child keeps the layout's encoding."""
    s = gpu_session
    draw, et, ew, enc = ELEM_CASES[name]
    rng = np.random.default_rng(11)
    lists = _random_lists(rng, N, lambda: draw(rng))
    if name == "int64_edges":
        lists[3] = [INT64_MIN, INT64_MAX, None]
    t = s.table([("k", T_INT, rng.integers(0, 1 << 40, N), None), ("xs", T_LIST, lists, None)])
    out, elem = _round_trip(s, t)
    assert elem[:2] == (et, ew) and elem[3] == 1, elem
    assert out.size == N and _list_bag(out) == _list_bag(t)
    st = _list_stats(out, "xs")
    assert (st["et"], st["enc"], st["nulls"]) == (et, enc, True), st
    # the received child is FOR-encoded where the layout said so: sending it
    # on reads it through the narrow encoding
    again, elem2 = _round_trip(s, out)
    assert elem2 == elem and _list_bag(again) == _list_bag(t)


@gpu
@pytest.mark.parametrize("values", [[INT64_MIN], [INT64_MIN, INT64_MIN + 10], [INT64_MIN, INT64_MIN + (1 << 31)]],
                         ids=["only_min", "min_within_2^24", "min_within_2^32"])
def test_round_trip_int64_min(gpu_session, values):
    """A minimum of INT64_MIN cannot be negated for the MAX all-reduce: the
    layout then takes the plain 8 bytes, whatever the maximum is."""
    s = gpu_session
    rng = np.random.default_rng(2)
    lists = _random_lists(rng, 101, lambda: values[int(rng.integers(0, len(values)))])
    t = s.table([("k", T_INT, np.arange(101), None), ("xs", T_LIST, lists, None)])
    out, elem = _round_trip(s, t)
    assert elem == (T_INT, 8, 0, 1), elem
    assert out.list_values("xs") == lists


@gpu
def test_null_lists_that_own_elements_send_none(gpu_session):
    """capf_table_add_list accepts a NULL list whose offsets give it elements.
    On the wire a NULL list has length 0: its elements stay out of the stream
    and of the counts, and the other lists keep theirs."""
    from capf_amd import _lib
    from capf_amd.table import GpuTable
    s = gpu_session
    n = 257
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 6, n)
    lens[0] = 3  # row 0: a NULL list owning three elements
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    vals = rng.integers(0, 1000, int(offs[-1]))
    valid = (rng.random(n) > 0.3).astype(np.uint8)
    valid[0], valid[1] = 0, 1
    assert ((valid == 0) & (lens > 0)).any()
    h = c_void_p()
    base = s.table([("k", T_INT, np.arange(n), None)])  # (kept: its handle is released with the object)
    _lib.call("capf_table_add_list", base._h, b"xs", T_INT, offs.ctypes.data, vals.ctypes.data, valid.ctypes.data,
              byref(h))
    t = GpuTable(s, h)
    want = [vals[offs[i]:offs[i + 1]].tolist() if valid[i] else None for i in range(n)]
    assert _list_stats(t, "xs")["n_elems"] == int(lens[valid.astype(bool)].sum())
    for parts in (1, 3):
        routed, counts = _route(s, t, ["k"], parts)
        rows, elem = _layout(routed)
        d_rows, d_el, ec = _pack(routed, counts, rows, elem)
        assert sum(ec) == int(lens[valid.astype(bool)].sum())
        out = _unpack(s, d_rows, d_el, rows, elem)
        order = out.column_arrays("k")[0].tolist()
        assert out.list_values("xs") == [want[r] for r in order]
        assert out.list_arrays("xs")[1][-1] == sum(ec)  # the receiver's NULL lists own nothing


@gpu
def test_round_trip_null_typed_elements(gpu_session):
    """`[null, null]` lists: no element bytes travel, only the lengths; the
    receiver rebuilds a NULL-typed child of the summed length."""
    s = gpu_session
    rng = np.random.default_rng(5)
    lists = _random_lists(rng, N, lambda: None, null_elems=False)
    t = s.table([("k", T_INT, np.arange(N), None), ("xs", T_LIST, lists, None)])
    assert _list_stats(t, "xs")["et"] == T_NULL
    out, elem = _round_trip(s, t)
    assert elem == (T_NULL, 0, 0, 0)
    assert out.list_values("xs") == t.list_values("xs")
    assert _list_stats(out, "xs")["et"] == T_NULL
    # a rank whose elements are NULL-typed adopts the others' type: they go out as NULL INTEGER elements
    routed, counts = _route(s, t, ["k"], 1)
    rows, _ = _layout(routed)
    d_rows, d_el, ec = _pack(routed, counts, rows, (T_INT, 3, 0, 1))
    adopted = _unpack(s, d_rows, d_el, rows, (T_INT, 3, 0, 1))
    assert _list_stats(adopted, "xs")["et"] == T_INT and adopted.list_values("xs") == t.list_values("xs")


@gpu
@pytest.mark.parametrize("shape", ["no_rows", "all_empty", "one_long", "past_grid_cap", "past_grid_cap_plain8",
                                   "past_group_grid_cap"])
def test_round_trip_shapes(gpu_session, shape):
    """0 rows; only empty lists; one list of 70,001 elements among short ones
    (work is divided by element, not by list); 2^20 + 3 elements in total, one
    sweep more than the 4,096 × 256 grid at one element per thread (the 8-byte
    records without validity are packed that way: `plain8`); 2^22 + 3 elements,
    one sweep more at the four records per thread of the other layouts."""
    s = gpu_session
    rng = np.random.default_rng(3)
    if shape == "no_rows":
        lists = []
    elif shape == "all_empty":
        lists = [[] for _ in range(N)]
    elif shape == "one_long":
        lists = _random_lists(rng, 257, lambda: int(rng.integers(0, 1 << 20)))
        lists[100] = rng.integers(0, 1 << 20, 70_001).tolist()
        lists[100][69_999] = None
    else:
        total, n = ((1 << 22) if shape == "past_group_grid_cap" else (1 << 20)) + 3, 65_537
        lens = np.full(n, total // n)
        lens[:total - lens.sum()] += 1
        wide = shape == "past_grid_cap_plain8"
        vals = rng.integers(-(1 << 62), 1 << 62, total) if wide else rng.integers(-(1 << 30), 1 << 30, total)
    if shape.startswith("past_"):
        # (built from arrays: a million-element Python list round trip is not the test)
        from capf_amd import _lib
        from capf_amd.table import GpuTable
        offs = np.zeros(n + 1, np.int64)
        offs[1:] = np.cumsum(lens)
        ev = None if wide else (rng.random(total) > 0.01).astype(np.uint8)
        base = s.table([("k", T_INT, np.arange(n), None)])
        h = c_void_p()
        _lib.call("capf_table_add_list_nulls", base._h, b"xs", T_INT, offs.ctypes.data, vals.ctypes.data, None,
                  ev.ctypes.data if ev is not None else None, byref(h))
        t = GpuTable(s, h)
    else:
        t = s.table([("k", T_INT, np.arange(len(lists)), None), ("xs", T_LIST, lists, None)], nrows=len(lists))
    out, elem = _round_trip(s, t)
    assert out.size == t.size
    a, b = t.list_arrays("xs"), out.list_arrays("xs")
    assert (a[1] == b[1]).all() and (a[3].astype(bool) == b[3].astype(bool)).all()  # offsets, list validity
    if a[4] is None:
        assert b[4] is None and (a[2] == b[2]).all()
    else:
        assert (a[4] == b[4]).all() and (a[2][a[4].astype(bool)] == b[2][a[4].astype(bool)]).all()
    if shape.startswith("past_"):
        assert b[1][-1] == total and elem[1:] == ((8, 0, 0) if wide else (4, elem[2], 1))
        assert _list_stats(out, "xs")["enc"] == (ENC_PLAIN if wide else ENC_FOR32)
    if shape == "one_long":
        assert _list_stats(out, "xs")["longest"] == 70_001


# ------------------------------------------------------------ routing
@gpu
def test_routing_carries_lists(gpu_session):
    """capf_table_hash_route with a LIST column aboard, parts 1, 2, 3 and 8:
    owners as oracle/route.py, each row's list still its own, the element
    counts per destination = numpy's sums of lengths per owner, and each
    destination's block (its slice of the rows and of the element stream)
    decodes to that owner's rows in stable order."""
    from oracle import route
    s = gpu_session
    rng = np.random.default_rng(7)
    ids = rng.integers(0, 1 << 22, N)
    lists = _random_lists(rng, N, lambda: int(rng.integers(0, 1 << 30)))
    lens = np.array([len(x) if x else 0 for x in lists])
    t = s.table([("k", T_INT, ids, None), ("row", T_INT, np.arange(N), None), ("xs", T_LIST, lists, None)])
    want_lists = t.list_values("xs")
    bits = [route.key_bits("int", ids, np.ones(N, bool))]
    for parts in (1, 2, 3, 8):
        want = route.owners(bits, N, parts)
        routed, counts = _route(s, t, ["k"], parts)
        assert counts == np.bincount(want, minlength=parts).tolist()
        order = np.argsort(want, kind="stable")
        rows = np.asarray(routed.column_arrays("row")[0])
        assert (rows == order).all()
        got_lists = routed.list_values("xs")
        assert got_lists == [want_lists[r] for r in rows]
        layout_rows, elem = _layout(routed)
        d_rows, d_el, ec = _pack(routed, counts, layout_rows, elem)
        assert ec == [int(lens[want == p].sum()) for p in range(parts)]
        r0 = e0 = 0
        for p in range(parts):
            block = _unpack(s, d_rows[r0:r0 + counts[p]], d_el[e0:e0 + ec[p]], layout_rows, elem)
            mine = order[want[order] == p]
            assert block.column_arrays("k")[0].tolist() == ids[mine].tolist()
            assert block.list_values("xs") == [want_lists[r] for r in mine]
            r0, e0 = r0 + counts[p], e0 + ec[p]


# ------------------------------------------------------------ errors
@gpu
def test_bad_arguments_are_illegal_argument(gpu_session):
    import torch
    from capf_amd import _lib
    s = gpu_session
    lists = [[1, None, 3], None, [], [4]]
    t = s.table([("k", T_INT, [1, 2, 3, 4], None), ("xs", T_LIST, lists, None)])
    Bad = _lib.IllegalArgumentException
    ec, rec = (c_int64 * 2)(), c_int32()

    def pack_elems(col, counts, et, ew, eb, en):
        _lib.call("capf_table_pack_list_elems", t._h, col.encode(), len(counts), (c_int64 * len(counts))(*counts),
                  et, ew, eb, en, ec, byref(rec), None)

    pack_elems("xs", [3, 1], T_INT, 3, 1, 1)  # the good call
    assert list(ec) == [3, 1] and rec.value == 4
    for counts in ([3, 2], [1, 1], [5, -1]):  # row counts that do not sum to the rows
        with pytest.raises(Bad):
            pack_elems("xs", counts, T_INT, 3, 1, 1)
    for et, ew in ((T_INT, 1), (T_INT, 0), (T_FLOAT, 4), (T_BOOL, 8), (T_NULL, 3), (T_LIST, 4), (9, 8)):
        with pytest.raises(Bad):  # a width that does not fit the element type
            pack_elems("xs", [4, 0], et, ew, 0, 1)
    with pytest.raises(Bad):  # INTEGER elements named as another type
        pack_elems("xs", [4, 0], T_FLOAT, 8, 0, 1)
    with pytest.raises(Bad):  # NULL elements without their validity byte
        pack_elems("xs", [4, 0], T_INT, 3, 1, 0)
    with pytest.raises(Bad):  # a scalar column named as a LIST column
        pack_elems("k", [4, 0], T_INT, 3, 1, 1)
    W = c_int32()
    for w in (3, 1, 0):  # a LIST column packed with a scalar's width
        with pytest.raises(Bad):
            _lib.call("capf_table_pack_rows", t._h, 1, _lib.strs(["xs"]), (c_int32 * 1)(w), (c_int64 * 1)(0),
                      (c_int32 * 1)(1), byref(W), None)
    with pytest.raises(Bad):  # a NULL list without the row's validity byte
        _lib.call("capf_table_pack_rows", t._h, 1, _lib.strs(["xs"]), (c_int32 * 1)(4), (c_int64 * 1)(0),
                  (c_int32 * 1)(0), byref(W), None)
    h = c_void_p()
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(Bad):  # a LIST column through the scalar-only entry point
        _lib.call("capf_table_from_packed_rows", s._h, 1, _lib.strs(["xs"]), (c_int32 * 1)(T_LIST), (c_int32 * 1)(4),
                  (c_int64 * 1)(0), (c_int32 * 1)(0), c_void_p(d.data_ptr()), 2, byref(h))

    def from_lists(types, nlists, n_elems, ew=3):
        _lib.call("capf_table_from_packed_lists", s._h, 1, _lib.strs(["xs"]), (c_int32 * 1)(*types), (c_int32 * 1)(4),
                  (c_int64 * 1)(0), (c_int32 * 1)(0), c_void_p(d.data_ptr()), 2, nlists, (c_int32 * 1)(T_INT),
                  (c_int32 * 1)(ew), (c_int64 * 1)(0), (c_int32 * 1)(0), (c_void_p * 1)(d.data_ptr()),
                  (c_int64 * 1)(n_elems), byref(h))

    from_lists([T_LIST], 1, 0)  # two rows of length 0, no elements: fine
    with pytest.raises(Bad):  # the lengths (0 + 0) do not sum to the stream's 5 records
        from_lists([T_LIST], 1, 5)
    with pytest.raises(Bad):  # a LIST column without its stream
        from_lists([T_LIST], 0, 0)
    with pytest.raises(Bad):  # an element width that fits no INTEGER
        from_lists([T_LIST], 1, 0, ew=2)
    with pytest.raises(Bad):  # a LIST column as a routing key
        _route(s, t, ["xs"], 2)
    with pytest.raises(Bad):
        _route(s, t, ["k", "xs"], 2)


# ------------------------------------------------------------ declarations (no GPU)
def test_jni_and_scala_declarations_agree():
    """The three entry points are declared in the header, bound in the JNI
    adapter (arrays length-checked before use) and declared @native with the
    same shapes; the Scala twin calls them and no longer refuses LIST columns."""
    import okapi_scala_scan as sc
    srcs = sc.integration_sources()
    native, twin = sc.strip_comments(srcs["Native.scala"]), sc.strip_comments(srcs["DistGpuTable.scala"])
    shim = open(os.path.join(ROOT, "integration", "jni", "capf_jni.cpp")).read()
    header = open(os.path.join(ROOT, "include", "capf_gpu.h")).read()
    for c_name, jni in (("capf_table_list_stats", "tableListStats"),
                        ("capf_table_pack_list_elems", "tablePackListElems"),
                        ("capf_table_from_packed_lists", "tableFromPackedLists")):
        assert re.search(rf"^capf_status {c_name}\(", header, re.M), c_name
        assert re.search(rf"^JNI\(\w+, {jni}\)", shim, re.M) and f"{c_name}(" in shim, jni
        assert re.search(rf"@native\s+def\s+{jni}\(", native), jni
        assert f"Native.{jni}(" in twin, jni
    assert re.search(r"@native\s+def\s+tableListStats\(table:\s*Long,\s*col:\s*String,\s*out:\s*Array\[Long\]\):\s*Unit",
                     native)
    assert re.search(r"@native\s+def\s+tablePackListElems\(table:\s*Long,\s*col:\s*String,\s*rowCounts:\s*Array\[Long\],"
                     r"\s*elemType:\s*Int,\s*width:\s*Int,\s*base:\s*Long,\s*elemNullable:\s*Int,"
                     r"\s*elemCountsOut:\s*Array\[Long\],\s*dOut:\s*Long\):\s*Int", native)
    assert re.search(r"@native\s+def\s+tableFromPackedLists\(session:\s*Long,\s*names:\s*Array\[String\],"
                     r"\s*types:\s*Array\[Int\],\s*width:\s*Array\[Int\],\s*base:\s*Array\[Long\],"
                     r"\s*nullable:\s*Array\[Int\],\s*dRows:\s*Long,\s*nrows:\s*Long,\s*elemTypes:\s*Array\[Int\],"
                     r"\s*elemWidth:\s*Array\[Int\],\s*elemBase:\s*Array\[Long\],\s*elemNullable:\s*Array\[Int\],"
                     r"\s*dElems:\s*Array\[Long\],\s*nElems:\s*Array\[Long\]\):\s*Long", native)
    # the adapter checks its arrays' lengths before it fills or reads them
    body = shim[shim.index("JNI(void, tableListStats)"):shim.index("JNI(void, tableDownloadDevice)")]
    assert "GetArrayLength(out) < 8" in body and "GetArrayLength(elemCountsOut)" in body
    assert body.count("illegal_argument(") >= 4
    assert "not moved between ranks" not in twin
    assert "TypeDate" in twin and "TypeLocalDateTime" in twin


# ------------------------------------------------------------ width selection (no GPU)
def test_int64_min_takes_the_plain_width():
    """range_entries → MAX over ranks → value_width, the path of _layout: a
    rank whose minimum is INT64_MIN forces 8 bytes, alone or beside a rank
    with a narrow range, whatever its own maximum."""
    from capf_amd.dist_table import range_entries, scalar_wire, value_width
    big = INT64_MAX
    assert range_entries(0, -1, 0) == (-big, -big) and range_entries(-5, 7, 3) == (5, 7)
    others = [None, range_entries(0, -1, 0), range_entries(100, 200, 5), range_entries(INT64_MIN + 1, INT64_MIN + 9, 2)]
    for mx in (INT64_MIN, INT64_MIN + (1 << 24) - 1, INT64_MIN + (1 << 32) - 1, 0, INT64_MAX):
        mine = range_entries(INT64_MIN, mx, 4)
        assert all(-big - 1 <= v <= big for v in mine)  # fits the int64 vector
        for other in others:
            lo = max(mine[0], other[0]) if other else mine[0]
            hi = max(mine[1], other[1]) if other else mine[1]
            assert value_width(-lo, hi) == (8, 0), (mx, other)
            assert scalar_wire(T_INT, -lo, hi) == (8, 0) and scalar_wire(6, -lo, hi) == (8, 0)
    # one above INT64_MIN negates exactly and keeps the narrow widths
    lo, hi = range_entries(INT64_MIN + 1, INT64_MIN + 1 + (1 << 24) - 1, 2)
    assert value_width(-lo, hi) == (3, INT64_MIN + 1)


def test_width_and_length_field_selection():
    from capf_amd.dist_table import length_width, scalar_wire, value_width
    assert value_width(5, 5 + (1 << 24) - 1) == (3, 5)
    assert value_width(5, 5 + (1 << 24)) == (4, 5)
    assert value_width(-7, -7 + (1 << 32) - 1) == (4, -7)
    assert value_width(-7, -7 + (1 << 32)) == (8, 0)
    assert value_width(INT64_MIN, INT64_MAX) == (8, 0)
    assert value_width(0, -1) == (3, 0)  # no value anywhere
    assert value_width(INT64_MAX, -INT64_MAX) == (3, 0)  # the all-reduce's "no value" entries
    assert length_width(0) == 4 and length_width((1 << 31) - 1) == 4 and length_width(1 << 31) == 8
    for t in (T_INT, T_STRING, 6, 7):  # DATE and LOCALDATETIME travel like INTEGER
        assert scalar_wire(t, 10, 20) == (3, 10)
    assert scalar_wire(T_FLOAT, 0, -1) == (8, 0) and scalar_wire(T_BOOL, 0, -1) == (1, 0)
    assert scalar_wire(T_NULL, 0, -1) == (0, 0)
