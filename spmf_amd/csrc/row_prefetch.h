// row_prefetch.h -- which entry words of a row the row pass touches ahead of time (row_pass.hip, issue_next).
//
// A row's entry words are contiguous, n words from a wave-uniform address of any 4-byte alignment.  The row pass
// vector-loads the first min(n, 128) of them one row before it works on the row; one row earlier still it reads
// single words of that window by scalar loads, so that its lines are in L2 when the vector load asks for them.  The
// words are a fixed ladder, kRowWarmStep apart, plus the window's last word: whatever the alignment of the row's
// start, every aligned unit of kRowWarmStep words that the window touches holds a rung or the last word
// (tools/row_prefetch_host.cpp enumerates it).  The step is 16 words: one load per 64-byte HALF of a 128-byte line.
// A load per whole line (32) measured slower than no warm-up at all, the half-line ladder 0.06 ms faster on C3
// (profiles/r09_row_prefetch_ab.txt): a scalar load brings in the half it names.
// Every index is a word of the row itself: nothing is read outside [0, n), nothing is rounded down to a line
// boundary, and the caller reads nothing for n = 0.
//
// Plain C++ (the host check compiles it without a device compiler).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPMF_HD __host__ __device__
#else
#define SPMF_HD
#endif

namespace spmf {

// words between two rungs (a build switch for the A/B: 32 = one per 128-byte line)
#ifndef ROW_PREFETCH_WORDS
#define ROW_PREFETCH_WORDS 16
#endif
constexpr int kRowWarmWindow = 128;                                  // the words the vector load of a row's issue point asks for
constexpr int kRowWarmStep = ROW_PREFETCH_WORDS;
constexpr int kRowWarmLoads = kRowWarmWindow / kRowWarmStep + 1;     // the rungs and the window's last word
static_assert(kRowWarmStep > 0 && kRowWarmStep <= 32 && kRowWarmWindow % kRowWarmStep == 0,
              "a rung per line at least: at most 32 words apart");

// word of the i-th warm-up load of a row of n > 0 entry words, i = 0 ... kRowWarmLoads - 1: in [0, n)
SPMF_HD inline int row_warm_word(int i, int n) {
  const int last = (n < kRowWarmWindow ? n : kRowWarmWindow) - 1;
  const int w = i < kRowWarmLoads - 1 ? i * kRowWarmStep : last;
  return w < last ? w : last;
}

}  // namespace spmf
