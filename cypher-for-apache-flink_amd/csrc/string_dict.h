// string_dict.h — the session's string dictionary and everything derived from it.
//
// A STRING column holds codes; the dictionary maps code ↔ string, append-only,
// on the host.  StringDict owns the strings and every device structure computed
// from them — the derived tables, the heap, and the state and locks of the
// match tables and the hash index (filled by strings.hip / string_fn.hip) —
// and is the only code that touches them.
//
// Lifetime rule: a table or heap buffer is replaced when it is rebuilt or
// grown, and sessions are used from several threads.  Every accessor hands out
// the BufPtr (taken under the lock), never a raw pointer, and the caller holds
// it until the launches that read it are enqueued: a prepared program keeps
// every dictionary buffer it reads (DeviceProgram::keep).  A buffer dropped
// then goes back to the stream-ordered block cache, behind those launches.
//
// Lock order: `mu` (strings, tables, heap) is a leaf, no other lock is taken
// while it is held.  match_mu and index_mu guard a whole step of strings.hip /
// string_fn.hip, which calls heap(), heap_append() and bytes_of() with its
// lock held: match_mu | index_mu → mu.  Those two are never held together.
#pragma once
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace capf {

struct Session;
struct DevBuf;
using BufPtr = std::shared_ptr<DevBuf>;

// The strings on the device: int64 offsets [n + 1] and the UTF-8 / WTF-8 bytes
// back to back, no terminators.  The bytes buffer is padded so that aligned
// 4-byte words covering any string, and one word ahead, may be read.
struct StringHeap {
  BufPtr off, bytes;
  int64_t nbytes;
  size_t n;  // strings covered
};

constexpr size_t STR_MATCH_TABLES = 16;  // cached match tables per session

class StringDict {
 public:
  explicit StringDict(Session *session) : s(session) {}

  // ---- host dictionary
  int64_t intern(const char *str);
  const char *lookup(int64_t code, const char *unknown = nullptr);  // unknown code: `unknown`, or throws when null
  size_t size();
  void digest(int64_t *count, uint64_t *fnv);  // FNV-1a over the strings in code order, 0xff between them
  // Σ bytes of the strings codes[0, n) (null: the codes c0 + i), those outside
  // [0, below) skipped — the profile's byte counts
  double bytes_of(const int64_t *codes, int64_t c0, int64_t n, int64_t below);
  bool empty(int64_t code) { return bytes_of(nullptr, code, 1, code + 1) == 0; }  // is string `code` ""?

  // ---- derived tables: one mechanism (string_dict.cpp TABLES).  A table has
  // rows() = max(n, 1) rows of its element, laid out as planes:
  //   LEN   int64 UTF-16 length                                  (CAPF_OP_STR_LEN)
  //   BOOL  uint8 0 false / 1 true / 2 neither                   (CAPF_OP_TO_BOOLEAN)
  //   NUM   [double rows][int64 rows][uint8 flags rows], bit 0: a DOUBLE,
  //         bit 1: an INTEGER                                    (CAPF_OP_STR_TO_NUM)
  //   RANK  [int64 rank rows][int64 order rows]: the rank in UTF-16 code-unit
  //         order (Java String.compareTo) and its inverse        (CAPF_OP_STR_RANK)
  enum TableId { LEN, BOOL, NUM, RANK, N_TABLES };
  struct Table {
    BufPtr buf;
    size_t n = 0;  // strings covered
    size_t rows() const { return n > 0 ? n : 1; }
  };
  Table table(TableId id);

  // ---- device heap.  heap() uploads only the strings interned since its last call.
  StringHeap heap();
  // The strings a device step made against the snapshot h, as codes h.n,
  // h.n + 1, …: n_new end offsets (absolute, from h.nbytes on) and nb bytes,
  // on the device and copied to the host.  While the dictionary still holds
  // h.n strings they are appended to the heap device to device and to the host
  // dictionary; when another thread interned meanwhile, each is resolved
  // through the host map instead (the heap catches up at its next use).
  // codes[r] = the code of new string r.
  void heap_append(const StringHeap &h, const int64_t *d_offs, const uint8_t *d_bytes, const int64_t *h_offs,
                   const char *h_bytes, int64_t n_new, int64_t nb, std::vector<int64_t> &codes);

  // Room for `need` elements of `elem` bytes in buf (`cap` now; the lock guarding buf held):
  // geometric from min_cap, the first `used` elements move device to device.
  void reserve(BufPtr &buf, size_t &cap, size_t need, size_t min_cap, size_t elem, size_t used);

  // ---- match tables (strings.hip), under match_mu: one uint8 (0 / 1) per
  // code, per (kind, pattern code); oldest first, at most STR_MATCH_TABLES
  struct MatchTable {
    int32_t kind;
    int64_t pattern;
    BufPtr buf;
    size_t n, cap;  // codes covered, capacity
  };
  std::mutex match_mu;
  std::vector<MatchTable> match_tables;

  // ---- hash index (string_fn.hip), under index_mu: an open-addressed table of codes (−1
  // empty, `slots` a power of two, at most half full) keyed by the 64-bit hash of each string's
  // bytes, and those hashes by code; extended over new codes, rebuilt when past half full
  struct Index {
    BufPtr tab, hashes;
    size_t n = 0, slots = 0, hash_cap = 0;  // codes covered, table slots, hashes allocated
  };
  std::mutex index_mu;
  Index index;

 private:
  Session *s;
  std::mutex mu;
  std::vector<std::string> strings;
  std::unordered_map<std::string, int64_t> string_codes;
  Table tables[N_TABLES];
  BufPtr d_heap_off, d_heap_bytes;
  size_t d_heap_n = 0, d_heap_nbytes = 0, d_heap_off_cap = 0, d_heap_bytes_cap = 0;
  void heap_reserve(size_t m, size_t end);  // room for m strings of `end` bytes in all (mu held)
};

}  // namespace capf
