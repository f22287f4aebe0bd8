// The workspace protocol of every entry point that takes (void* ws, size_t ws_bytes), written once (host code only; included from common.hpp).
//   layout   one function per entry point, size_t x_carve(WsCarver c, <shape>, XWs* out), takes its arrays from the carver in order, each rounded
//            up to 256 bytes, and returns c.bytes().  The sizer runs it on a null base, x_carve({}, ..): it only measures; the call on the
//            caller's pointer, x_carve({(char*)ws, 0}, ..): the two cannot disagree.
//   refusal  SDK_REQUIRE_WS: null, short, misaligned, in that order, each with its own message, each returning 2 before anything is written
//            or enqueued.
#pragma once
#include <stddef.h>
#include <stdint.h>

inline size_t ws_round(size_t v) { return (v + 255) & ~(size_t)255; }

struct WsCarver {
  char* base;
  size_t off;
  // count elements of T at the current offset (nullptr when measuring: no pointer is ever formed from a null base).  count * sizeof(T) is within
  // size_t for every argument the sizers accept: their range checks are the guard, not this
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += ws_round(count * sizeof(T));
    return p;
  }
  size_t bytes() const { return off; }
};

// -> 0, or 2 with sdk_last_error set.  align: what the entry point requires of ws (1: nothing)
inline int ws_refused(const char* fn, const char* sizer, const void* ws, size_t ws_bytes, size_t need, int align) {
  if (!ws) sdk_set_error("%s: null workspace (%zu bytes needed, %s)", fn, need, sizer);
  else if (ws_bytes < need) sdk_set_error("%s: workspace of %zu bytes, %zu needed (%s)", fn, ws_bytes, need, sizer);
  else if ((uintptr_t)ws % (uintptr_t)align) sdk_set_error("%s: ws=%p must be %d-byte aligned", fn, ws, align);
  else return 0;
  return 2;
}
#define SDK_REQUIRE_WS(fn, sizer, ws, ws_bytes, need, align)                 \
  do {                                                                       \
    if (ws_refused(fn, sizer, ws, ws_bytes, need, align)) return 2;          \
  } while (0)
