// rtx_film_sampled.h — films for the light-sampling estimators (rtx_film_create_sampled,
// include/rtx.h; DESIGN.md §4j "Sampled films"): the frames of rtx_render_nee / rtx_render_mis
// kept as a film, fixed spp or with the reference's per-pixel adaptive sampling.
// Included once, by rtx_queries.hip, after rtx_nee.h.  The path kernel below is the frame form of
// k_sampled (rtx_nee.h) behind the active list: the same camera_slot, nee_path and slot_write.
//
// Contract: sample k of subset pixel i has the value of the k_sampled<.., CAMERA = true, MIS> slot of
// (seed, global pixel index, sample k): camera_slot (get_ray on stream 0), nee_path<.., MIS>,
// sum + L_end.  A fixed film adds its samples to `sum` in sample order from 0; an adaptive film records them in
// sample order with k_accumulate's arithmetic (RecordSample, then IsConverged from min_spp on) and
// stops a pixel at its first converged sample or at the budget; a sample traced past that point is
// discarded.  Work is done in groups: G samples of every entry of an active list of subset indices
// (no list: every pixel of the subset), traced by k_film_paths into the scene's slot scratch and
// replayed by k_film_record, which also marks the entries that go on; k_film_emit compacts those
// into the next list in ascending subset order (rtx_scan's prefix).  The state does not depend on G.
#pragma once

#include "rtx_nee.h"

namespace rtxd {

// One launch over entries [e0, e0 + ne) of a group.  Every read of `list` is bounded twice: by
// `bound`, which the host vouches for (at most the list's capacity, npix), and by the device
// count the kernel that wrote the list left beside it.
struct FilmGroup {
  const uint32_t* list;   // the active list (subset indices, ascending), or null: entry e is subset pixel e
  const uint32_t* count;  // entries of `list` (device word; not read with a null list)
  uint32_t bound;         // entries at most: <= npix
  uint32_t e0, ne;        // this launch's entries
  uint32_t G;             // samples per entry: slot j is sample s0 + j % G of entry e0 + j / G
  int32_t s0;
  int32_t max_depth;
  uint32_t npix;          // pixels of the subset (the film's state arrays)
  uint64_t seed;
  double* L;              // 3 doubles per slot of the launch
  uint32_t* segs;         // segments per slot
};

// Entry e's subset pixel; false for an entry outside the list (or a list value outside the film).
__device__ __forceinline__ bool film_entry(const FilmGroup& A, uint32_t e, uint32_t& p) {
  uint32_t n = A.bound;
  if (A.list) n = min(n, *A.count);
  if (e >= n) return false;
  p = A.list ? A.list[e] : e;
  return p < A.npix;
}

// One lane per slot, k_sampled's launch shape and its camera-form body for the slot's (pixel, sample);
// a kernel of its own because the pixel comes through the active list.
template <int STACK, bool FAST, bool MIS>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_film_paths(DScene S, EmitterTable E, NeeCamera cam,
                                                                    FilmGroup A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.ne * A.G) return;
  const uint32_t r = j / A.G, k = j - r * A.G;
  uint32_t i;
  if (!film_entry(A, A.e0 + r, i)) return;
  const uint32_t smp = (uint32_t)A.s0 + k;
  uint32_t pix;
  V3 o, d;
  camera_slot(cam, A.seed, i, smp, pix, o, d);
  const NeePath p = nee_path<STACK, FAST, MIS>(S, E, A.seed, pix, smp, A.max_depth, o, d, stk, NeeNoRecord{});
  slot_write(A.L, A.segs, j, p.sum + p.L_end, p.closest + p.shadow);
}

// Counters every wave of a launch adds to: spread over kFilmSpread words kFilmSpreadStride words
// apart, as spread_add's are (rtx_frame_kernels.h); k_film_totals sums them.  (spread_add counts a
// wave's non-zero lanes with a ballot, film_spread_sum adds the lanes' 64-bit values: two reductions,
// so the two keep their own definitions, and the frame kernels' header is not this unit's.)
constexpr int kFilmSpread = 64, kFilmSpreadStride = 16;
constexpr int kFilmCtrTraced = 0, kFilmCtrRecorded = kFilmSpread * kFilmSpreadStride,
              kFilmCtrTotals = 2 * kFilmSpread * kFilmSpreadStride,  // traced, recorded
    kFilmCtrWords = kFilmCtrTotals + 4;                               // ... then the two lists' counts (u32 each)
__device__ __forceinline__ void film_spread_sum(unsigned long long* base, unsigned long long v) {
  for (int m = 32; m >= 1; m >>= 1) v += (unsigned long long)__shfl_xor((long long)v, m);
  if (v && lane_id() == 0) atomicAdd(base + (blockIdx.x % kFilmSpread) * kFilmSpreadStride, v);
}

struct FilmRecord {
  int32_t min_spp, budget;
  double rel;
  uint32_t* keep;            // adaptive: per entry of the list, 1 when it goes on (neither converged nor at the budget)
  unsigned long long* ctr;   // kFilmCtrWords
};

// One lane per entry of the launch: its G slot values replayed in sample order into the film's
// state.  Fixed films: a plain sum.  Adaptive films: k_accumulate's loop body per sample
// (RecordSample, pixel_state.h:22-39; IsConverged, :54-72, once the pixel holds min_spp samples),
// division and square roots as written there.  G may be 0: the pass only marks who goes on.
template <bool ADAPTIVE>
__global__ __launch_bounds__(kBlock) void k_film_record(PixelSoA px, FilmGroup A, FilmRecord R) {
  const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const int64_t npix = (int64_t)A.npix;
  uint32_t p = 0;
  const bool in_launch = i < A.ne;
  const bool live = in_launch && film_entry(A, A.e0 + i, p);
  unsigned long long traced = 0, recorded = 0;
  uint32_t kp = 0;
  if (live) {
    const double* L = A.L + 3 * (uint64_t)i * A.G;
    const uint32_t* sg = A.segs + (uint64_t)i * A.G;
    for (uint32_t k = 0; k < A.G; k++) traced += sg[k];
    if (ADAPTIVE) {
      if (!px.conv[p]) {
        double sum[3], mean[3], m2[3];
        for (int c = 0; c < 3; c++) sum[c] = px.sum[c * npix + p], mean[c] = px.mean[c * npix + p], m2[c] = px.m2[c * npix + p];
        int n = px.samples[p];
        bool conv = false;
        for (uint32_t k = 0; k < A.G && !conv && n < R.budget; k++) {
          const double* x = L + 3 * (uint64_t)k;
          n++;
          for (int c = 0; c < 3; c++) {
            double mu = mean[c];
            double delta = x[c] - mu;
            mu += delta / n;
            double delta2 = x[c] - mu;
            mean[c] = mu;
            m2[c] += delta2 * delta;
          }
          for (int c = 0; c < 3; c++) sum[c] += x[c];
          if (n >= R.min_spp) {
            bool ok = true;
            for (int c = 0; c < 3 && ok; c++) {
              double var = n > 1 ? m2[c] / (n - 1) : 0.0;
              double mu = fmax(fabs(mean[c]), 1e-3);
              double err = sqrt(var) / sqrt((double)n);
              if (err / mu > R.rel) ok = false;
            }
            conv = ok;
          }
          recorded += sg[k];
        }
        for (int c = 0; c < 3; c++) px.sum[c * npix + p] = sum[c], px.mean[c * npix + p] = mean[c], px.m2[c * npix + p] = m2[c];
        px.samples[p] = n;
        px.conv[p] = conv;
        kp = !conv && n < R.budget ? 1u : 0u;
      }
    } else {
      double sum[3];
      for (int c = 0; c < 3; c++) sum[c] = px.sum[c * npix + p];
      for (uint32_t k = 0; k < A.G; k++)
        for (int c = 0; c < 3; c++) sum[c] += L[3 * (uint64_t)k + c];
      for (int c = 0; c < 3; c++) px.sum[c * npix + p] = sum[c];
      px.samples[p] += (int32_t)A.G;
      recorded = traced;
    }
  }
  if (ADAPTIVE && in_launch) R.keep[A.e0 + i] = kp;  // (e0 + ne <= bound <= the flags' capacity)
  film_spread_sum(R.ctr + kFilmCtrTraced, traced);
  film_spread_sum(R.ctr + kFilmCtrRecorded, recorded);
}

// The next active list: entry e of the group just recorded goes to place (low word of pk[e],
// exclusive_scan_packed of keep) when keep[e]; the last entry leaves the count.  `list` is read
// only where keep is set, and k_film_record sets it only below the list's own count.
__global__ __launch_bounds__(kBlock) void k_film_emit(const uint32_t* __restrict__ list,
                                                      const uint32_t* __restrict__ keep,
                                                      const uint64_t* __restrict__ pk, uint32_t bound, uint32_t cap_out,
                                                      uint32_t* __restrict__ next, uint32_t* __restrict__ next_count) {
  const uint32_t e = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (e >= bound) return;
  const uint32_t at = (uint32_t)pk[e], k = keep[e];
  if (k && at < cap_out) next[at] = list ? list[e] : e;
  if (e == bound - 1) *next_count = min(at + (k ? 1u : 0u), cap_out);
}

// One wave: the spread counters summed into ctr[kFilmCtrTotals], [+ 1].
__global__ __launch_bounds__(64) void k_film_totals(unsigned long long* ctr) {
  static_assert(kFilmSpread == 64, "one spread counter per lane");
  unsigned long long t = ctr[kFilmCtrTraced + lane_id() * kFilmSpreadStride];
  unsigned long long r = ctr[kFilmCtrRecorded + lane_id() * kFilmSpreadStride];
  for (int m = 32; m >= 1; m >>= 1) {
    t += (unsigned long long)__shfl_xor((long long)t, m);
    r += (unsigned long long)__shfl_xor((long long)r, m);
  }
  if (lane_id() == 0) ctr[kFilmCtrTotals] = t, ctr[kFilmCtrTotals + 1] = r;
}

}  // namespace rtxd
