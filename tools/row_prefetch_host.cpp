// Host check of the row pass's warm-up address rule (spmf_amd/csrc/row_prefetch.h: row_warm_word).
//
// For every row length n = 0 ... 300 and every alignment of the row's first word inside a 128-byte line (32 of them):
//   - every index the rule returns is a word of the row, 0 <= w < n (nothing is read in front of or behind it);
//   - every 128-byte line that the first min(n, 128) words span holds one of them, and so does every aligned unit
//     of the ladder's own step (16 words: every 64-byte half line).
// A row of n = 0 is never given to the rule (the kernel reads nothing for it): the program checks that it spans no
// line and asks for nothing.  Built with -fsanitize=address,undefined and run on the CPU by
// tests/test_row_prefetch_host.py, with the default step and with -DROW_PREFETCH_WORDS=32 (the build variant).
#include <cstdio>
#include <vector>

#include "row_prefetch.h"

int main() {
  using namespace spmf;
  const int units[2] = {32, kRowWarmStep};  // words of a 128-byte line, and of the unit the ladder is meant to hit
  long checked = 0, loads = 0;
  for (int n = 0; n <= 300; ++n) {
    const int window = n < kRowWarmWindow ? n : kRowWarmWindow;
    for (int align = 0; align < 32; ++align) {
      // absolute word numbers: the row starts at word 1024 + align of a line-aligned array
      const long start = 1024 + align;
      std::vector<long> hit;                // the absolute words asked for
      if (n > 0) {
        for (int i = 0; i < kRowWarmLoads; ++i) {
          const int w = row_warm_word(i, n);
          if (w < 0 || w >= n) {
            std::printf("FAIL n=%d align=%d load %d: word %d outside [0, %d)\n", n, align, i, w, n);
            return 1;
          }
          if (w >= window) {
            std::printf("FAIL n=%d align=%d load %d: word %d behind the window of %d\n", n, align, i, w, window);
            return 1;
          }
          hit.push_back(start + w);
          ++loads;
        }
      }
      if (window > 0) {
        for (int line : units) {
          for (long l = start / line; l <= (start + window - 1) / line; ++l) {
            bool found = false;
            for (long h : hit) found = found || h / line == l;
            if (!found) {
              std::printf("FAIL n=%d align=%d: unit %ld (of %d words) of the window is not touched\n", n, align,
                          l - start / line, line);
              return 1;
            }
          }
        }
      } else if (!hit.empty()) {
        std::printf("FAIL n=0 align=%d: a row without entries asks for a word\n", align);
        return 1;
      }
      ++checked;
    }
  }
  std::printf("ok: %ld (n, alignment) cases, %ld loads, %d loads per row, %d words apart\n", checked, loads,
              kRowWarmLoads, kRowWarmStep);
  return 0;
}
