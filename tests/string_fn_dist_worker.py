"""The rank process of tests/test_string_fn_device.py's distributed case (a
module of its own: a spawned process imports its target's module before the
package is on the path)."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def subjects():
    """1,000 distinct strings, a third of them with a non-ASCII character (the
    host's share of toUpper)."""
    return [f"Value {i:04d} straße"[:10 + i % 9] for i in range(1000)]


def worker(rank, world, port, q):
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CAPF_STR_FN="device")
    os.environ.pop("CAPF_STR_LONG", None)
    import traceback
    from ctypes import byref, c_int64, c_uint64
    import torch
    import torch.distributed as dist
    try:
        import capf_import  # noqa: F401
        import capf_amd.table as tb
        from capf_amd import _lib
        from capf_amd.dist_table import DistSession, GpuExchange
        from capf_amd.expr import T_INT, T_STRING, ToUpper, Var
        from capf_amd.header import RecordHeader
        from capf_amd.table import GpuSession
        tb.CODE_MAP_MAX, tb.VALUE_MAP_MAX = 4, 8  # the value-map path, past its old cap
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        s = GpuSession.on_torch_stream(0)
        s.set_profiling(True)
        ds = DistSession(s, GpuExchange(s))
        subj = subjects()
        full = s.table([("s", T_STRING, subj, None), ("k", T_INT, list(range(len(subj))), None)])
        shard = ds.shard(full, "k")  # each rank keeps the rows it owns: different distinct values
        mine = shard.local.column_values("s")
        h = RecordHeader({Var("s"): "s", Var("k"): "k"})
        out = shard.withColumns((ToUpper(Var("s")), "x"), header=h, params={})
        rows = sorted(zip(out.column_values("k"), out.column_values("x")))
        cnt, dig = c_int64(), c_uint64()
        _lib.call("capf_string_digest", s._h, byref(cnt), byref(dig))
        q.put((rank, rows, len(mine), cnt.value, dig.value, s.profile().get("str_fn_len", {}).get("launches", 0)))
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001 - report, do not hang the parent
        q.put((rank, traceback.format_exc(), None, None, None, None))
