"""Kernel rates of the LIST element packer and unpacker of the exchange
(csrc/shuffle.hip: k_pack_elems / k_pack_elems8, k_unpack_elems) on one GPU.

    python tools/list_exchange_timing.py [--out FILE] [--reps N] [--log2-elems E]

Workload: one LIST<INTEGER> column of 2^E elements (E = 24 by default) in
2^(E−4) lists, the elements spread over the lists evenly at random (mean
length 16).  Four element layouts: values whose range fits 24 bits (3-byte
records, FOR24 on the receiver) and values over the whole int64 range (8-byte
records), each with and without NULL elements (one more validity byte per
record: 4 and 9 bytes).

Timed, with session profiling on (device events around each kernel, read per
run): `pack_elems` inside capf_table_pack_list_elems and `unpack_elems` inside
capf_table_from_packed_lists.  Without a validity byte the records ARE the
receiver's element buffer and unpack_elems is one device-to-device copy.
The yardstick is the `pack_rows` kernel (k_pack_rows, unchanged by the LIST
work for scalar columns) packing a one-column INTEGER table of 2^E rows in the
same layout: the same number of output bytes.

bytes = records × record size, the packed side only (what KernelTimer books for
pack_rows): the reads on the other side (8 B or 3 B per value, 1 B validity)
are not counted, in either kernel.  Medians of --reps runs after two warm-up
runs of the same shape in the same process; min and max beside them.  Every
round trip is checked against the uploaded arrays before it is timed.  One
JSON line per measurement goes to stdout; --out writes the table."""
import argparse
import json
import os
import statistics
import sys
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_INT, T_LIST = 1, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--log2-elems", type=int, default=24)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import capf_import
    capf_import.load()
    from capf_amd import _lib
    from capf_amd.dist_table import length_width, scalar_wire
    from capf_amd.table import GpuSession, GpuTable

    s = GpuSession(0)
    rng = np.random.default_rng(24)
    total = 1 << args.log2_elems
    n = total >> 4
    lens = rng.multinomial(total, np.full(n, 1.0 / n)).astype(np.int64)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    rows_tab = s.table([("k", T_INT, np.arange(n), None)])

    def kernel_ms(name, fn):
        """Per-run device time of kernel `name` inside fn(): 2 warm-ups, then --reps runs."""
        out = []
        for i in range(2 + args.reps):
            s.reset_profile()
            keep = fn()
            s.sync()
            prof = s.profile()
            assert name in prof and prof[name]["launches"] == 1, (name, sorted(prof))
            if i >= 2:
                out.append(prof[name]["total_ms"])
            del keep
        return out

    results = []
    s.set_profiling(True)
    for label, lo, hi in (("for24", 1000, 1000 + (1 << 24) - 1), ("int64", -(1 << 62), 1 << 62)):
        vals = rng.integers(lo, hi, total, dtype=np.int64, endpoint=True)
        vals[0], vals[-1] = lo, hi
        for with_valid in (False, True):
            ev = (rng.random(total) > 0.05).astype(np.uint8) if with_valid else None
            h = c_void_p()
            if with_valid:
                _lib.call("capf_table_add_list_nulls", rows_tab._h, b"xs", T_INT, offs.ctypes.data, vals.ctypes.data,
                          None, ev.ctypes.data, byref(h))
            else:
                _lib.call("capf_table_add_list", rows_tab._h, b"xs", T_INT, offs.ctypes.data, vals.ctypes.data, None,
                          byref(h))
            t = GpuTable(s, h)
            vmin = int(vals[ev.astype(bool)].min()) if with_valid else lo
            vmax = int(vals[ev.astype(bool)].max()) if with_valid else hi
            ew, eb = scalar_wire(T_INT, vmin, vmax)
            en = int(with_valid)
            rec = ew + en
            assert ew == (3 if label == "for24" else 8)
            # ---- element pack
            ec, rb = (c_int64 * 1)(), c_int32()
            d_el = torch.empty(total * rec, dtype=torch.uint8, device="cuda")
            pack_args = (t._h, b"xs", 1, (c_int64 * 1)(n), T_INT, ew, eb, en, ec, byref(rb), c_void_p(d_el.data_ptr()))
            _lib.call("capf_table_pack_list_elems", *pack_args)
            assert ec[0] == total and rb.value == rec
            # ---- rows (length field only) and the receiver
            lw = length_width(int(lens.max()))
            cols, w1, b1, n1 = _lib.strs(["xs"]), (c_int32 * 1)(lw), (c_int64 * 1)(0), (c_int32 * 1)(0)
            W = c_int32()
            d_rows = torch.empty(n * lw, dtype=torch.uint8, device="cuda")
            _lib.call("capf_table_pack_rows", t._h, 1, cols, w1, b1, n1, byref(W), c_void_p(d_rows.data_ptr()))

            def unpack():
                out = c_void_p()
                _lib.call("capf_table_from_packed_lists", s._h, 1, cols, (c_int32 * 1)(T_LIST), w1, b1, n1,
                          c_void_p(d_rows.data_ptr()), n, 1, (c_int32 * 1)(T_INT), (c_int32 * 1)(ew),
                          (c_int64 * 1)(eb), (c_int32 * 1)(en), (c_void_p * 1)(d_el.data_ptr()), (c_int64 * 1)(total),
                          byref(out))
                return GpuTable(s, out)

            # the round trip is right before anything is timed
            et, o2, v2, ok2, ev2 = unpack().list_arrays("xs")
            assert (o2 == offs).all() and ok2.all()
            if with_valid:
                m = ev.astype(bool)
                assert (ev2 == ev).all() and (v2[m] == vals[m]).all()
            else:
                assert ev2 is None and (v2 == vals).all()
            pack_ms = kernel_ms("pack_elems", lambda: _lib.call("capf_table_pack_list_elems", *pack_args))
            unpack_ms = kernel_ms("unpack_elems", unpack)
            # ---- yardstick: pack_rows of a scalar table with the same output bytes
            sv = s.table([("v", T_INT, vals, ev)])
            d_out = torch.empty(total * rec, dtype=torch.uint8, device="cuda")
            yard_args = (sv._h, 1, _lib.strs(["v"]), (c_int32 * 1)(ew), (c_int64 * 1)(eb), (c_int32 * 1)(en), byref(W),
                         c_void_p(d_out.data_ptr()))
            _lib.call("capf_table_pack_rows", *yard_args)
            assert W.value == rec and torch.equal(d_out, d_el)  # the same record, byte for byte
            yard_ms = kernel_ms("pack_rows", lambda: _lib.call("capf_table_pack_rows", *yard_args))
            for kernel, ms in (("pack_elems", pack_ms), ("unpack_elems", unpack_ms), ("pack_rows (yardstick)", yard_ms)):
                med = statistics.median(ms)
                r = {"layout": label, "validity": with_valid, "record_bytes": rec, "kernel": kernel,
                     "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                     "bytes": total * rec, "gb_per_s": round(total * rec / med / 1e6, 1)}
                results.append(r)
                print(json.dumps(r), flush=True)
            del t, sv, d_el, d_out
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"elements 2^{args.log2_elems} in {n} lists (mean 16), reps {args.reps} after 2 warm-ups; "
                    "kernel times from device events (session profiling)\n")
            f.write("layout  validity  record B  kernel                   median ms     min      max        bytes"
                    "     GB/s   vs pack_rows\n")
            for i, r in enumerate(results):
                yard = results[i - i % 3 + 2]
                f.write(f"{r['layout']:<7} {str(r['validity']):<9} {r['record_bytes']:>8}  {r['kernel']:<24}"
                        f"{r['median_ms']:>10.4f} {r['min_ms']:>8.4f} {r['max_ms']:>8.4f} {r['bytes']:>12}"
                        f" {r['gb_per_s']:>8.1f} {r['gb_per_s'] / yard['gb_per_s']:>10.2f}x\n")


if __name__ == "__main__":
    main()
