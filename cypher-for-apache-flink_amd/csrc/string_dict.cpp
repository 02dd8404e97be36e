// string_dict.cpp — the session's string dictionary (string_dict.h).
#include <algorithm>

#include "capf_internal.h"
#include "string_parse.h"

namespace capf {

using Lock = std::lock_guard<std::mutex>;

// ------------------------------------------------------------ host dictionary
int64_t StringDict::intern(const char *str) {
  Lock lk(mu);
  auto it = string_codes.find(str);
  if (it != string_codes.end()) return it->second;
  const int64_t c = (int64_t)strings.size();
  strings.emplace_back(str);
  string_codes.emplace(str, c);
  return c;
}

const char *StringDict::lookup(int64_t code, const char *unknown) {
  Lock lk(mu);
  if (code >= 0 && code < (int64_t)strings.size()) return strings[(size_t)code].c_str();
  if (!unknown) illegal("unknown string code");
  return unknown;
}

size_t StringDict::size() {
  Lock lk(mu);
  return strings.size();
}

void StringDict::digest(int64_t *count, uint64_t *fnv) {
  Lock lk(mu);
  uint64_t h = 1469598103934665603ull;
  for (const std::string &str : strings) {
    for (unsigned char ch : str) h = (h ^ ch) * 1099511628211ull;
    h = (h ^ 0xffu) * 1099511628211ull;  // separator: ("ab","c") != ("a","bc")
  }
  *count = (int64_t)strings.size();
  *fnv = h;
}

double StringDict::bytes_of(const int64_t *codes, int64_t c0, int64_t n, int64_t below) {
  Lock lk(mu);
  double by = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t c = codes ? codes[i] : c0 + i;
    if (c >= 0 && c < below) by += (double)strings[(size_t)c].size();
  }
  return by;
}

// ------------------------------------------------------------ derived tables
// `elem` bytes per string, every byte `fill` until `put` writes string i's
// element(s) into the m-row planes at t, or `all` the whole dictionary's (one sort).
struct TableSpec {
  size_t elem, fill;
  void (*put)(const std::string &str, size_t i, size_t m, uint8_t *t);
  void (*all)(const std::vector<std::string> &strings, size_t m, uint8_t *t);
};

static void put_len(const std::string &str, size_t i, size_t, uint8_t *t) { ((int64_t *)t)[i] = utf16_length(str); }
static void put_bool(const std::string &str, size_t i, size_t, uint8_t *t) { t[i] = parse_bool(str); }
static void put_num(const std::string &str, size_t i, size_t m, uint8_t *t) {
  double d = 0;
  int64_t v = 0;
  if (parse_java_double(str, &d)) ((double *)t)[i] = d, t[16 * m + i] |= 1;
  if (parse_int32(str, &v)) ((int64_t *)(t + 8 * m))[i] = v, t[16 * m + i] |= 2;
}
static void all_ranks(const std::vector<std::string> &strings, size_t m, uint8_t *t) {
  int64_t *rank = (int64_t *)t, *order = rank + m;
  for (size_t i = 0; i < strings.size(); ++i) order[i] = (int64_t)i;
  std::sort(order, order + strings.size(),
            [&](int64_t x, int64_t y) { return utf16_cmp(strings[(size_t)x], strings[(size_t)y]) < 0; });
  for (size_t r = 0; r < strings.size(); ++r) rank[(size_t)order[r]] = (int64_t)r;
}

static const TableSpec TABLES[StringDict::N_TABLES] = {
    /* LEN  */ {8, 0, put_len, nullptr},
    /* BOOL */ {1, 2, put_bool, nullptr},
    /* NUM  */ {17, 0, put_num, nullptr},
    /* RANK */ {16, 0, nullptr, all_ranks},
};

StringDict::Table StringDict::table(TableId id) {
  Lock lk(mu);
  Table &t = tables[id];
  if (t.n != strings.size() || !t.buf) {  // the dictionary grew: built again, whole
    const TableSpec &spec = TABLES[id];
    const size_t m = std::max<size_t>(strings.size(), 1);
    std::vector<uint8_t> host(m * spec.elem, (uint8_t)spec.fill);
    if (spec.all) spec.all(strings, m, host.data());
    else
      for (size_t i = 0; i < strings.size(); ++i) spec.put(strings[i], i, m, host.data());
    t.buf = s->alloc(host.size());
    HIP_CHECK(hipMemcpyAsync(t.buf->p, host.data(), host.size(), hipMemcpyHostToDevice, s->stream));
    s->sync();  // the pageable source
    t.n = strings.size();
  }
  return t;
}

// ------------------------------------------------------------ device heap
void StringDict::reserve(BufPtr &buf, size_t &cap, size_t need, size_t min_cap, size_t elem, size_t used) {
  if (need <= cap) return;
  const size_t grown = std::max(2 * cap, std::max(need, min_cap));
  BufPtr nb = s->alloc(elem * grown);
  if (buf && used > 0) HIP_CHECK(hipMemcpyAsync(nb->p, buf->p, elem * used, hipMemcpyDeviceToDevice, s->stream));
  buf = nb;
  cap = grown;
}

constexpr size_t HEAP_PAD = 16;  // bytes kept past the last string (StringHeap)

void StringDict::heap_reserve(size_t m, size_t end) {
  reserve(d_heap_off, d_heap_off_cap, m + 1, 1024, 8, d_heap_n + 1);
  reserve(d_heap_bytes, d_heap_bytes_cap, end + HEAP_PAD, 1 << 16, 1, d_heap_nbytes);
}

StringHeap StringDict::heap() {
  Lock lk(mu);
  const size_t m = strings.size();
  if (m > d_heap_n || !d_heap_off) {
    // the new strings' offsets (and offset 0 the first time) and bytes
    std::vector<int64_t> off;
    std::string bytes;
    if (!d_heap_off) off.push_back(0);
    size_t end = d_heap_nbytes;
    for (size_t i = d_heap_n; i < m; ++i) {
      bytes += strings[i];
      end += strings[i].size();
      off.push_back((int64_t)end);
    }
    heap_reserve(m, end);
    const size_t first = m + 1 - off.size();  // index of the first offset uploaded
    HIP_CHECK(hipMemcpyAsync((int64_t *)d_heap_off->p + first, off.data(), 8 * off.size(), hipMemcpyHostToDevice,
                             s->stream));
    if (!bytes.empty())
      HIP_CHECK(hipMemcpyAsync((uint8_t *)d_heap_bytes->p + (end - bytes.size()), bytes.data(), bytes.size(),
                               hipMemcpyHostToDevice, s->stream));
    s->sync();  // the pageable sources
    d_heap_n = m;
    d_heap_nbytes = end;
  }
  return StringHeap{d_heap_off, d_heap_bytes, (int64_t)d_heap_nbytes, d_heap_n};
}

void StringDict::heap_append(const StringHeap &h, const int64_t *d_offs, const uint8_t *d_bytes, const int64_t *h_offs,
                             const char *h_bytes, int64_t n_new, int64_t nb, std::vector<int64_t> &codes) {
  const size_t n0 = h.n;
  const int64_t base = h.nbytes;
  codes.resize((size_t)n_new);
  Lock lk(mu);
  const bool same = strings.size() == n0 && d_heap_off && d_heap_n == n0 && (int64_t)d_heap_nbytes == base;
  if (same) {  // codes n0.. in order; the heap grows device to device
    heap_reserve(n0 + (size_t)n_new, (size_t)(base + nb));
    HIP_CHECK(hipMemcpyAsync((int64_t *)d_heap_off->p + n0 + 1, d_offs, 8 * (size_t)n_new, hipMemcpyDeviceToDevice,
                             s->stream));
    if (nb > 0)
      HIP_CHECK(hipMemcpyAsync((uint8_t *)d_heap_bytes->p + base, d_bytes, (size_t)nb, hipMemcpyDeviceToDevice,
                               s->stream));
    d_heap_n = n0 + (size_t)n_new;
    d_heap_nbytes = (size_t)(base + nb);
  }
  int64_t b = base;
  for (int64_t r = 0; r < n_new; ++r) {
    std::string str(h_bytes + (b - base), (size_t)(h_offs[r] - b));
    b = h_offs[r];
    auto it = same ? string_codes.end() : string_codes.find(str);
    if (it != string_codes.end()) {
      codes[(size_t)r] = it->second;
      continue;
    }
    codes[(size_t)r] = (int64_t)strings.size();
    string_codes.emplace(str, codes[(size_t)r]);
    strings.push_back(std::move(str));
  }
}

}  // namespace capf
