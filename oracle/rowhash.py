"""numpy restatement of csrc/kernels_hash.hip hash_row / table_capacity — TEST
INFRASTRUCTURE ONLY.

For ONE key column holding a non-NULL INTEGER w the hash table's row hash is
fmix64(0x243F6A8885A308D3 ^ w), fmix64 the murmur3 finaliser of
csrc/device_common.h, and the home slot is hash & (capacity − 1).  Tests use
it to pick keys whose linear-probe chains wrap past the last slot.  Whoever
changes hash_row (csrc/kernels_hash.hip) changes this file too."""
import numpy as np

SEED = 0x243F6A8885A308D3


def fmix64(k):
    k = np.asarray(k).astype(np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xFF51AFD7ED558CCD)
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xC4CEB9FE1A85EC53)
        k = k ^ (k >> np.uint64(33))
    return k


def hash_row(w):
    """Row hash of one non-NULL INTEGER key column (int64 values)."""
    return fmix64(np.asarray(w, dtype=np.int64).view(np.uint64) ^ np.uint64(SEED))


def table_capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def home_slot(w, n_rows):
    """Home slot of each key in the table built over n_rows rows."""
    return (hash_row(w) & np.uint64(table_capacity(n_rows) - 1)).astype(np.int64)
