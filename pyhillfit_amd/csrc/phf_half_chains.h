/* phf_half_chains.h — how a chain of N rows splits into two half-chains: the one rule behind the device's split-R-hat, ESS, batch
 * means and correlations (phf_diagnostics.hip, phf_batch_means.hip, phf_comoments.hip) and their host twins.  h = floor(N/2);
 * half 0 = rows 0..h-1, half 1 = the last h rows; the middle row of an odd N belongs to neither.  Plain C, integers only. */
#ifndef PHF_HALF_CHAINS_H
#define PHF_HALF_CHAINS_H

#include <stdint.h>

#ifndef PHF_HD
#if defined(__HIPCC__)
#define PHF_HD static __host__ __device__ __forceinline__
#else
#define PHF_HD static inline __attribute__((always_inline))
#endif
#endif

/* which half row n of N belongs to, and its index m there; -1: the dropped middle row of an odd N */
PHF_HD int phf_half_of(int64_t total_rows, int64_t n, int64_t* m) {
  const int64_t h = total_rows / 2;
  if (n < h) { *m = n; return 0; }
  if (n >= total_rows - h) { *m = n - (total_rows - h); return 1; }
  *m = 0;
  return -1;
}

/* the rows of a call that fall into one half: rows offset .. offset + nr - 1 of the call's rows are rows m0 .. of the half;
 * closes: the half's last row is among them */
typedef struct {
  int64_t offset, nr, m0;
  int closes;
} phf_half_segment;

/* cut the call's rows [first_row, first_row + num_rows) of N at `half`: 0 when none of them falls into it */
PHF_HD int phf_half_cut(int64_t total_rows, int64_t first_row, int64_t num_rows, int half, phf_half_segment* s) {
  const int64_t h = total_rows / 2;
  const int64_t begin = half == 0 ? 0 : total_rows - h, hend = begin + h, end = first_row + num_rows;
  const int64_t lo = first_row > begin ? first_row : begin, hi = end < hend ? end : hend;
  if (lo >= hi) return 0;
  s->offset = lo - first_row;
  s->nr = hi - lo;
  s->m0 = lo - begin;
  s->closes = hi == hend;
  return 1;
}

#endif /* PHF_HALF_CHAINS_H */
