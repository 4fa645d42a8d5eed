// arena.h -- host only: how the library divides memory a caller hands it (the step's workspace, a streaming
// call's scratch, the layout builder's two buffers) into its device buffers.
//
// A layout function takes an Arena and the struct its pointers land in, and names every buffer once:
//     T.Ap = a.take<float>(S * D * KP);
// On an Arena without memory it only counts: `used` is then what the public size function returns.  On the
// caller's memory and byte count the same run binds and checks: `used` beyond the count means too small, and
// from the region that does not fit on every pointer is null.  One function is the size, the check and the
// binding, so the three cannot list different buffers.
#pragma once
#include <stddef.h>

namespace spmf {

struct Arena {
  char* base = nullptr;    // 256-byte aligned, or null: count only
  size_t bytes = 0;        // what the caller says base holds
  size_t used = 0;
  Arena() = default;
  Arena(void* memory, size_t bytes) : base((char*)memory), bytes(bytes) {}
  // the next region: n elements of T, rounded up to whole 256-byte lines; null where it does not fit
  template <typename T>
  T* take(size_t n) {
    const size_t at = used;
    used += (n * sizeof(T) + 255) & ~(size_t)255;
    return base && used <= bytes ? (T*)(base + at) : nullptr;
  }
  bool fits() const { return used <= bytes; }
};

}  // namespace spmf
