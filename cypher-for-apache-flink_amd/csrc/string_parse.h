// string_parse.h — what a dictionary string is as a length, a BOOLEAN, a number
// and a sort key (host only).
//
// The strings are UTF-8, or WTF-8 where Java handed over a lone surrogate;
// lengths and order are java.lang.String's (UTF-16 code units), the casts Flink
// SQL's.  The dictionary's derived device tables (string_dict.cpp) are filled from these.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

namespace capf {

// Java String.length of a UTF-8 string: UTF-16 code units (one per code point,
// two above U+FFFF)
inline int64_t utf16_length(const std::string &u) {
  int64_t n = 0;
  for (size_t i = 0; i < u.size(); ++i) {
    const unsigned char c = (unsigned char)u[i];
    if ((c & 0xC0) == 0x80) continue;  // continuation byte
    n += c >= 0xF0 ? 2 : 1;
  }
  return n;
}

// Flink's CAST(string AS BOOLEAN) (FlinkSQLExprMapper.scala:185): 'true' /
// 'false' in any case, surrounding blanks ignored; anything else is NULL
inline uint8_t parse_bool(const std::string &u) {
  size_t b = 0, e = u.size();
  while (b < e && (unsigned char)u[b] <= ' ') ++b;
  while (e > b && (unsigned char)u[e - 1] <= ' ') --e;
  std::string t = u.substr(b, e - b);
  for (auto &ch : t) ch = (char)std::tolower((unsigned char)ch);
  return t == "true" ? 1 : t == "false" ? 0 : 2;
}

// CAST(string AS DOUBLE): java.lang.Double.valueOf after String.trim —
// [+-] (NaN | Infinity | digits[.digits] | .digits)([eE][+-]digits)? [fFdD]?
inline bool parse_java_double(const std::string &u, double *out) {
  size_t b = 0, e = u.size();
  while (b < e && (unsigned char)u[b] <= ' ') ++b;
  while (e > b && (unsigned char)u[e - 1] <= ' ') --e;
  std::string t = u.substr(b, e - b);
  if (t.empty()) return false;
  size_t i = 0;
  if (t[i] == '+' || t[i] == '-') ++i;
  const std::string rest = t.substr(i);
  if (rest == "NaN" || rest == "Infinity") {
    *out = rest == "NaN" ? std::nan("") : (t[0] == '-' ? -HUGE_VAL : HUGE_VAL);
    return true;
  }
  size_t nd = 0;
  while (i < t.size() && isdigit((unsigned char)t[i])) ++i, ++nd;
  if (i < t.size() && t[i] == '.') {
    ++i;
    while (i < t.size() && isdigit((unsigned char)t[i])) ++i, ++nd;
  }
  if (nd == 0) return false;
  if (i < t.size() && (t[i] == 'e' || t[i] == 'E')) {
    ++i;
    if (i < t.size() && (t[i] == '+' || t[i] == '-')) ++i;
    size_t ne = 0;
    while (i < t.size() && isdigit((unsigned char)t[i])) ++i, ++ne;
    if (ne == 0) return false;
  }
  const size_t num_end = i;
  if (i < t.size() && strchr("fFdD", t[i])) ++i;
  if (i != t.size()) return false;
  *out = strtod(t.substr(0, num_end).c_str(), nullptr);
  return true;
}

// CAST(string AS INT), the semantics the reference expectations pin
// (FunctionTests.scala:1101-1152): a decimal integer after trim, a fractional
// part truncated ('82.9' -> 82), within 32 bits; anything else NULL
inline bool parse_int32(const std::string &u, int64_t *out) {
  size_t b = 0, e = u.size();
  while (b < e && (unsigned char)u[b] <= ' ') ++b;
  while (e > b && (unsigned char)u[e - 1] <= ' ') --e;
  size_t i = b;
  bool neg = false;
  if (i < e && (u[i] == '+' || u[i] == '-')) neg = u[i++] == '-';
  int64_t v = 0;
  size_t nd = 0;
  while (i < e && isdigit((unsigned char)u[i])) {
    v = v * 10 + (u[i++] - '0');
    if (v > (int64_t)1 << 32) v = (int64_t)1 << 32;  // saturate: out of range below
    ++nd;
  }
  if (nd == 0) return false;
  if (i < e && u[i] == '.') {
    ++i;
    while (i < e && isdigit((unsigned char)u[i])) ++i;
  }
  if (i != e) return false;
  if (neg) v = -v;
  if (v < -2147483648LL || v > 2147483647LL) return false;
  *out = v;
  return true;
}

// Java String.compareTo order: UTF-16 code units.  On UTF-8 bytes that is
// code-point order except that a supplementary character (4 bytes, a
// surrogate pair D800-DBFF first) sorts below U+E000-U+FFFF (3 bytes EE-EF).
inline int utf16_cmp(const std::string &a, const std::string &b) {
  auto key = [](const std::string &u, size_t &i) -> uint32_t {  // next code unit class
    const unsigned char c = (unsigned char)u[i];
    size_t len = c < 0x80 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
    uint32_t cp = c < 0x80 ? c : c < 0xE0 ? c & 0x1F : c < 0xF0 ? c & 0x0F : c & 0x07;
    for (size_t k = 1; k < len && i + k < u.size(); ++k) cp = cp << 6 | ((unsigned char)u[i + k] & 0x3F);
    i += len;
    return cp >= 0x10000 ? 0xD800 + ((cp - 0x10000) >> 10) : cp;  // the high surrogate
  };
  size_t i = 0, j = 0;
  while (i < a.size() && j < b.size()) {
    const size_t i0 = i, j0 = j;
    const uint32_t x = key(a, i), y = key(b, j);
    if (x != y) return x < y ? -1 : 1;
    if (x >= 0xD800 && x < 0xDC00) {  // equal high surrogates: compare the low ones
      std::string ca = a.substr(i0, i - i0), cb = b.substr(j0, j - j0);
      if (ca != cb) return ca < cb ? -1 : 1;  // same lead: byte order = low-surrogate order
    }
  }
  return i < a.size() ? 1 : (j < b.size() ? -1 : 0);
}

}  // namespace capf
