// rtx_capi.hip — C ABI (include/rtx.h) over the HIP kernels: scene upload and in-place updates,
// the frame renderer (full-path render, films, the denoiser's filter entry points, P3 encoding).
// What a scene needs decided and tabulated on the host before the upload (checks, the fast tree,
// the device tables) is plain C++ in rtx_scene_plan.cc.  The ray-query entry points (rtx_intersect*, rtx_occluded*, rtx_ao*, rtx_aov*, rtx_radiance*,
// rtx_irradiance*, rtx_direct*) are rtx_queries.hip; both units share rtx_host.h.  gfx950 only; no
// CPU compute path and no fallback: a missing device or a HIP error is returned as RTX_ERR_* with
// a message in rtx_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <atomic>
#include <chrono>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "rtx_host.h"
#include "rtx_refit.h"
#include "rtx_denoise.h"
#include "rtx_film.h"
#include "rtx_frame_kernels.h"
#include "rtx_p3.h"
#include "rtx_scan.h"
#include "rtx_scene_plan.h"

// The PARK instantiations of k_persistent are compiled in rtx_park.hip (RTX_PARK_TU).
namespace rtxd {
#define RTX_PARK_EXTERN(ST, CO, SC, MP, PK)                                                                   \
  extern template __global__ void k_persistent<ST, true, CO, SC, PK, -1, false, false, false, MP>(RenderArgs, \
                                                                                              unsigned long long*);
RTX_PARK_INSTANCES(RTX_PARK_EXTERN)
#undef RTX_PARK_EXTERN
#define RTX_PARK_TRI_EXTERN(ST, MP, PK)                                                                             \
  extern template __global__ void k_persistent<ST, true, false, false, PK, RTX_PRIM_TRIANGLE, false, false, false, \
                                               MP>(RenderArgs, unsigned long long*);                              \
  extern template __global__ void k_persistent<ST, true, false, false, PK, RTX_PRIM_TRIANGLE, true, false, false,  \
                                               MP>(RenderArgs, unsigned long long*);                              \
  extern template __global__ void k_persistent<ST, true, false, false, PK, RTX_PRIM_TRIANGLE, true, true, false,   \
                                               MP>(RenderArgs, unsigned long long*);
RTX_PARK_TRI_INSTANCES(RTX_PARK_TRI_EXTERN)
#undef RTX_PARK_TRI_EXTERN
}  // namespace rtxd

namespace {
thread_local std::string g_err;  // rtx_last_error()'s message (fail, rtx_host.h, sets it through rtx_internal_set_error)
}  // namespace
static_assert(rtxplan::kPlainGlobalSpheres == rtxd::kGlobalSpheres, "the planner's flag bit is the kernels'");

// statistics, queue counts, then the slot counter block (8 region counters 128 B apart, [128 + 4]
// the segment buffer (0), ...)
constexpr int kSlotBlockWords = 8 * 16 + 8;
constexpr int kCounterWords = 64 + kSlotBlockWords;

// Where a render's output goes once a band of it is final (fixed-spp renders): the
// accumulate of the last sample group runs in kBands bands of the frame's pixels, and after
// each one `copy` enqueues that band's device-to-host copy on the copy stream, so the
// framebuffer crosses PCIe while the next band is still being summed.  Band edges are
// multiples of `align` pixels (whole stripes of the caller's layout).
struct BandSink {
  int64_t align;
  int (*copy)(void* ctx, int64_t p0, int64_t p1, hipStream_t cs);
  void* ctx;
  // Adaptive renders: the caller's whole-image host framebuffer as the device sees it (pinned,
  // mapped), or nullptr.  With it, the output goes to the host early, while the last phases
  // still run (copy stream), and the pixels those phases change are written into it by the
  // device at the end (k_patch_host) instead of a second whole-frame copy.
  double* host_rgb_dev = nullptr;
};
constexpr int64_t kEarlyOutDiv = 32;  // the early output once a phase holds at most npix / 32 pixels (4: C3 / C4 adaptive -0.7 %, r9j / r9k)
constexpr int kBands = 8;  // bands of the last accumulate and of the D2H copies that overlap them (ab_bands_*: 2 / 4 / 8 / 16)

// Adaptive renders in phases (render_adaptive)
// render_adaptive: the smallest phase planned while pixels remain (round 3: 2^23; with the pooled
// prediction 2^21, scripts/adaptive_sim.py and r05 r8j / r8k)
constexpr int64_t kAdaptPhaseSlots = 1 << 21;
constexpr double kAdaptMarginStep = 0.25;      // render_adaptive: batch margin 1 + step * (phase - 1) (0.5: within noise, r3y)
// Overrides of the adaptive schedules' constants (0: the default): rtx_internal_adapt_tune, a
// test and tuning hook (not in rtx.h) that forces small workspaces and floors, so the paths
// that only a large frame at a large budget reaches run on small frames too.
struct AdaptTune {
  int64_t phase_slots;  // phases: the smallest phase planned while pixels remain (kAdaptPhaseSlots)
  int phase_kcap;       // phases: the largest batch of one pixel (else from the workspace)
  int first_map;         // the uniform first pass: 1 the phase kernel (block-shared chunks), 0 the uniform-group one (< 0: default)
  double phase_mstep;    // phases: the batch margin's growth per phase (< 0: kAdaptMarginStep)
  double margin1;        // the margin of the batches after the first phase (< 0: kAdaptMargin1)
  double pool_w;         // the pooled prediction's centre weight (< 0: kAdaptPoolW; 0: not pooled)
};
static AdaptTune g_tune{0, 0, -1, -1.0, -1.0, -1.0};
// adaptive early outputs so far (renders whose output went to the host while phases still ran)
// and the pixels k_patch_host rewrote: rtx_internal_early_output_stats, a test hook
static std::atomic<long long> g_early_outputs{0}, g_early_patched{0};
// render_adaptive: the margin of the batches after the first phase, and k_adapt_plan's centre
// weight (0: each pixel's own prediction only): ranked first by scripts/adaptive_sim.py, then
// C3 adaptive +4.0 %, C2 +0.5 % against the unpooled margin 1.0 (r05 r8j / r8k)
constexpr double kAdaptMargin1 = 0.8;
constexpr double kAdaptPoolW = 8.0;
constexpr int kFirstPassMap = 1;  // the adaptive first pass runs the phase kernel (MAP 1, no slot map)
// RTX_DEBUG_HOST: host-side timestamps of a frame (render_stripes_to_host prints them, with the
// device; per thread: rtx_render_multi renders each device on a thread of its own)
static const bool g_debug_host = std::getenv("RTX_DEBUG_HOST") != nullptr;
static double host_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static thread_local double g_t_launch = 0, g_t_sync0 = 0, g_t_sync1 = 0;
namespace {

// The allowance of a scene's slot buffers (the radiance records of the samples in flight, the
// wavefront's path queues, the adaptive workspaces): half of the device memory that is free or
// already held by them, so several scenes on one device, or a smaller GPU, get smaller groups
// instead of RTX_ERR_NOMEM.  ONE allowance for all of them: a render keeps the other kinds'
// buffers (and, for an adaptive render, the radiance buffer beyond its first pass) only while
// they fit beside its own (render_device_impl releases them otherwise) and sizes its own within
// the allowance minus what those kept buffers take.  The free-memory query is made once
// per scene (the first render that sizes its slots; it costs ~0.5 ms, too much per frame):
// scenes created later see what the earlier ones took.
double slot_allowance(rtx_scene* sc) {
  if (sc->slot_mem < 0) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
      (void)hipGetLastError();
      fr = (size_t)1 << 62;
    }
    double held = (double)sc->lbuf.n + (double)sc->queue[0].n + (double)sc->queue[1].n + (double)sc->segs1.n;
    held += (double)sc->aw.lbuf.n + (double)sc->aw.smap.n + (double)sc->aw.segs.n;
    sc->slot_mem = 0.5 * ((double)fr + held);
  }
  return sc->slot_mem;
}
// Slots a render keeps in flight: `want`, within the allowance less `other` bytes the render's
// other slot buffers take.
int64_t slot_target(rtx_scene* sc, int64_t bytes_per_slot, int64_t want, double other = 0.0) {
  const double mem = std::max(0.0, slot_allowance(sc) - other);
  return std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)(mem / (double)bytes_per_slot)));
}

int persistent_grid(rtx_scene* sc, const void* fn, size_t lds) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlock, lds) != hipSuccess || per_cu <= 0)
    per_cu = 1;
  return std::max(1, per_cu) * sc->cus;
}


struct Launch {
  rtx_scene* sc;
  hipStream_t s;
  int stack;
  bool fast, count;
  int park = 0;  // persistent: 0 plain kernel, PARK kernel (parked traversals) with 1 the leaf-step, 2 the speculative walk
  bool generic = false;  // RTX_FLAG_GENERIC: no per-scene specialisation (TK, LAMB, NOTEX, NODOF)
  int map = 0;           // k_persistent MAP: 0 uniform groups, 1 an adaptive phase's slot map
  mutable uint32_t build = 0;  // RTX_BUILD_* bits of the persistent instantiation launched last
};

template <int STACK, bool FAST, bool COUNT>
int run_extend(const Launch& L, const RenderArgs& A, const PathQueue& q, const unsigned* cnt, int64_t max_items) {
  const size_t lds = stack_lds_bytes(STACK);
  const int64_t need = (max_items + kBlock - 1) / kBlock;
  const int grid = (int)std::max<int64_t>(
      1, std::min<int64_t>(need, persistent_grid(L.sc, (const void*)k_wf_extend<STACK, FAST, COUNT>, lds)));
  hipLaunchKernelGGL((k_wf_extend<STACK, FAST, COUNT>), dim3(grid), dim3(kBlock), lds, L.s, A, q, cnt);
  HIPC(hipGetLastError());
  return RTX_OK;
}

template <int STACK, bool FAST, bool COUNT, bool SCATTER, int PARK, int TK, bool LAMB, bool NOTEX, bool NODOF,
          int MAP>
int run_persistent_k1(const Launch& L, const RenderArgs& A, unsigned long long* next_slot) {
  if (A.stack_slots < 1 || A.stack_slots > STACK + 1) return fail(RTX_ERR_INVALID, "bad traversal stack size");
  const size_t lds = persist_lds(A.stack_slots, spec_walk(PARK, FAST, SCATTER), block_region_kind(MAP, SCATTER)).end;
  int grid = persistent_grid(
      L.sc, (const void*)k_persistent<STACK, FAST, COUNT, SCATTER, PARK, TK, LAMB, NOTEX, NODOF, MAP>, lds);
  L.build = (PARK ? RTX_BUILD_PARK : 0u) | (PARK == 2 ? RTX_BUILD_SPECULATIVE : 0u) | (TK == (int)RTX_PRIM_SPHERE ? RTX_BUILD_SPHERE_TREE : 0u) |
            (TK == (int)RTX_PRIM_TRIANGLE ? RTX_BUILD_TRIANGLE_TREE : 0u) | (LAMB ? RTX_BUILD_LAMBERTIAN : 0u) |
            (NOTEX ? RTX_BUILD_NO_TEXTURES : 0u) | (NODOF ? RTX_BUILD_NO_DEFOCUS : 0u) |
            (FAST ? RTX_BUILD_FAST : 0u) | (COUNT ? RTX_BUILD_COUNT : 0u) | (SCATTER ? RTX_BUILD_SCATTER : 0u);
  if (std::getenv("RTX_DEBUG_LAUNCH"))
    fprintf(stderr, "rtx launch: k_persistent build 0x%x grid %d (%d blocks per CU) lds %zu B stack_slots %d\n",
            L.build, grid, grid / std::max(1, L.sc->cus), lds, A.stack_slots);
  hipLaunchKernelGGL((k_persistent<STACK, FAST, COUNT, SCATTER, PARK, TK, LAMB, NOTEX, NODOF, MAP>), dim3(grid),
                     dim3(kBlock), lds, L.s, A, next_slot);
  HIPC(hipGetLastError());
  return RTX_OK;
}
// adaptive renders draw their slots from a slot map (L.map; never with the scatter API)
template <int STACK, bool FAST, bool COUNT, bool SCATTER, int PARK, int TK, bool LAMB = false, bool NOTEX = false,
          bool NODOF = false>
int run_persistent_k0(const Launch& L, const RenderArgs& A, unsigned long long* next_slot) {
  if (!SCATTER && L.map == 1)
    return run_persistent_k1<STACK, FAST, COUNT, SCATTER, PARK, TK, LAMB, NOTEX, NODOF, SCATTER ? 0 : 1>(L, A, next_slot);
  if (L.map) return fail(RTX_ERR_INVALID, "slot maps are not used with the scatter API");
  return run_persistent_k1<STACK, FAST, COUNT, SCATTER, PARK, TK, LAMB, NOTEX, NODOF, 0>(L, A, next_slot);
}
// the texture-free plain build also comes without the camera's thin-lens sampling (defocus
// off; C2 +1.0 %; the PARK build lost 2.8 % with it, ab_nodof_*)
template <int STACK, bool FAST, bool COUNT, bool SCATTER, int PARK, int TK, bool LAMB = false, bool NOTEX = false>
int run_persistent_k(const Launch& L, const RenderArgs& A, unsigned long long* next_slot) {
  if (NOTEX && !PARK && A.cam.defocus_angle <= 0)
    return run_persistent_k0<STACK, FAST, COUNT, SCATTER, PARK, TK, LAMB, NOTEX, NOTEX && !PARK>(L, A, next_slot);
  return run_persistent_k0<STACK, FAST, COUNT, SCATTER, PARK, TK, LAMB, NOTEX>(L, A, next_slot);
}
// fast frames of a scene whose tree holds one kind run a build for that kind: triangles with
// the PARK schedule (the bunny), spheres with the plain one (the final and mixed scenes)
template <int STACK, bool FAST, bool COUNT, bool SCATTER, int PARK>
int run_persistent(const Launch& L, const RenderArgs& A, unsigned long long* next_slot) {
  constexpr bool spec = FAST && !COUNT && !SCATTER;
  constexpr int TK = spec ? (PARK ? (int)RTX_PRIM_TRIANGLE : (int)RTX_PRIM_SPHERE) : -1;
  if (TK >= 0 && A.S.tree_kind == TK && !L.generic) {
    // the triangle (PARK) build also comes for all-Lambertian scenes (the bunny)
    if (TK == (int)RTX_PRIM_TRIANGLE && A.S.all_lambertian) {
      constexpr bool tri = TK == (int)RTX_PRIM_TRIANGLE;
      if (A.S.no_textures) return run_persistent_k<STACK, FAST, COUNT, SCATTER, PARK, TK, tri, tri>(L, A, next_slot);
      return run_persistent_k<STACK, FAST, COUNT, SCATTER, PARK, TK, tri>(L, A, next_slot);
    }
    // the sphere (plain) build also comes for scenes that read no textures (the final scene)
    if (TK == (int)RTX_PRIM_SPHERE && A.S.no_textures)
      return run_persistent_k<STACK, FAST, COUNT, SCATTER, PARK, TK, false, TK == (int)RTX_PRIM_SPHERE>(L, A,
                                                                                                       next_slot);
    return run_persistent_k<STACK, FAST, COUNT, SCATTER, PARK, TK>(L, A, next_slot);
  }
  return run_persistent_k<STACK, FAST, COUNT, SCATTER, PARK, -1>(L, A, next_slot);
}

// template dispatch helpers
int extend(const Launch& L, const RenderArgs& A, const PathQueue& q, const unsigned* c, int64_t n) {
  return with_walk(L.stack, L.fast, [&](auto w) {
    return L.count ? run_extend<w.stack, w.fast, true>(L, A, q, c, n) : run_extend<w.stack, w.fast, false>(L, A, q, c, n);
  });
}
template <bool FAST, bool COUNT, bool SCATTER, int PARK>
int persist_s(const Launch& L, const RenderArgs& A, unsigned long long* ns) {
  return L.stack == 32 ? run_persistent<32, FAST, COUNT, SCATTER, PARK>(L, A, ns)
                       : run_persistent<64, FAST, COUNT, SCATTER, PARK>(L, A, ns);
}
template <bool SCATTER>
int persist_m(const Launch& L, const RenderArgs& A, unsigned long long* ns) {
  constexpr int kSpec = SCATTER ? 1 : 2;  // (the scatter API never runs the PARK kernel)
  if (L.fast && L.park == 2 && !SCATTER)
    return L.count ? persist_s<true, true, SCATTER, kSpec>(L, A, ns) : persist_s<true, false, SCATTER, kSpec>(L, A, ns);
  if (L.fast && L.park && !SCATTER)
    return L.count ? persist_s<true, true, SCATTER, 1>(L, A, ns) : persist_s<true, false, SCATTER, 1>(L, A, ns);
  if (L.fast)
    return L.count ? persist_s<true, true, SCATTER, 0>(L, A, ns) : persist_s<true, false, SCATTER, 0>(L, A, ns);
  return L.count ? persist_s<false, true, SCATTER, 0>(L, A, ns) : persist_s<false, false, SCATTER, 0>(L, A, ns);
}

int time_park_schedule(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, hipStream_t s);

// Bytes of an adaptive render's uniform first pass (min_spp samples of every pixel): its
// radiance records, and in counting renders their segment counts, in the scene's buffers.
double adaptive_first_bytes(int64_t npix, const rtx_render_params* prm, int budget, bool count) {
  const int K1 = std::min(std::max(1, prm->min_spp), budget);
  return (double)npix * K1 * (3 * sizeof(double) + (count ? 2 : 0));
}

// Counting renders: the persistent launch's slot counter block names the buffer its paths'
// segment counts go to (k_persistent COUNT builds read word 8 * 16 + 4 of it).
int set_segbuf(unsigned long long* ctr, uint16_t* segs, hipStream_t st) {
  const unsigned long long v = (unsigned long long)(uintptr_t)segs;
  uint32_t* w = (uint32_t*)(ctr + 8 * 16 + 4);  // (two 32-bit memsets: stream-ordered, no host staging)
  HIPC(hipMemsetD32Async((hipDeviceptr_t)w, (int)(uint32_t)v, 1, st));
  HIPC(hipMemsetD32Async((hipDeviceptr_t)(w + 1), (int)(uint32_t)(v >> 32), 1, st));
  return RTX_OK;
}
// Adaptive sampling on the persistent kernel: the reference's WavefrontRenderer::Render loop
// (wavefront.cc:57-225, always adaptive) with the same per-pixel results, on the caller's
// stream `s`.  Phase 1 traces min_spp samples of every pixel (one uniform launch) and
// k_adapt_record replays them and sizes each pixel's next batch.  After each phase, record +
// next batch sizes (k_adapt_record, k_adapt_floor); before each phase, prefix sum and slot map
// (k_adapt_expand); the host reads the next phase's slot count (one pinned word) to launch it
// or stop; every phase is a launch of its own with its own drain.
// `mark` records a hot-kernel timing event (before and after each persistent launch);
// hot_launches counts them.  The caller resolves the pixels (k_resolve).
// `trace(g, Lg, Ag, ctr, nslots)` fills phase g's nslots radiance records (Ag.L; slot p * Ag.K + k
// in phase 1, the slot map's (pixel, sample) afterwards): the persistent launch (trace_persistent)
// in renders, a gather from a caller's table in the test hook rtx_internal_adaptive_replay.
inline int trace_persistent(int, const Launch& Lg, const RenderArgs& Ag, unsigned long long* ctr, uint64_t) {
  return persist_m<false>(Lg, Ag, ctr);
}
template <class Mark, class Early, class Trace>
int render_adaptive(rtx_scene* sc, const Launch& L, const RenderArgs& A, const rtx_render_params* prm,
                    const PixelSoA& px, int budget, double other, hipStream_t s, Mark mark, uint64_t& hot_launches,
                    Early early, Trace trace) {
  const int64_t npix = A.npix;
  const int K1 = std::min(std::max(1, prm->min_spp), budget);
  static const bool debug = std::getenv("RTX_DEBUG_ADAPT") != nullptr;  // per-phase slot counts on stderr
  const int64_t phase_slots = g_tune.phase_slots > 0 ? g_tune.phase_slots : kAdaptPhaseSlots;
  if ((int64_t)npix * K1 > 0xFFFFFFFFll) return fail(RTX_ERR_INVALID, "adaptive render: npix x min_spp above 2^32");
  AdaptWs& w = sc->aw;
  int rc;
  // the uniform first pass's radiance (and segment) records, in the scene's buffers
  const double first_bytes = adaptive_first_bytes(npix, prm, budget, L.count);
  // slots after the first phase: 24 B of radiance + 8 B of slot map each (+ 2 B of segments),
  // within the allowance less the first pass and what the render keeps of other buffers
  const int64_t cap = std::min<int64_t>(
      0xFFFFFFFFll, slot_target(sc, 32 + (L.count ? 2 : 0), 1ll << kSlotTargetLog2, first_bytes + other));
  if (npix * 4 > cap) return fail(RTX_ERR_NOMEM, "adaptive render: too many pixels for the device memory");
  int32_t kcap = (int32_t)std::min<int64_t>(budget, std::max<int64_t>(4, (cap / npix) & ~3ll));
  if (g_tune.phase_kcap > 0) kcap = std::min(kcap, g_tune.phase_kcap);
  {
    const int64_t slots = npix * (int64_t)kcap;
    if ((rc = w.lbuf.reserve(slots * 3 * sizeof(double)))) return rc;
    if (L.count && (rc = w.segs.reserve(slots * sizeof(uint16_t)))) return rc;
    if ((rc = w.smap.reserve(slots * sizeof(uint2)))) return rc;
    for (DevBuf* b : {&w.lst[0], &w.lst[1], &w.kl[0], &w.kl[1], &w.ol[0], &w.ol[1], &w.knext})
      if ((rc = b->reserve(npix * sizeof(uint32_t)))) return rc;
    if ((rc = w.pk.reserve(npix * sizeof(unsigned long long)))) return rc;
    if ((rc = w.rv.reserve(npix * sizeof(float)))) return rc;
    if ((rc = w.scan_tmp.reserve(std::max<size_t>(16, rtxscan::temp_bytes_packed(npix))))) return rc;
    if ((rc = w.ctr.reserve(kAdaptCtrWords * sizeof(unsigned long long)))) return rc;
    if ((rc = w.total_h.reserve(2 * sizeof(unsigned long long)))) return rc;
    if (!w.ev) HIPC(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
  }
  unsigned long long* ctr = w.ctr.as<unsigned long long>();  // 8 region counters, then the slot count, ...
  // record + next batch sizes after phase g (its slots in Lph: the uniform first phase's, or the
  // phase's slot map; its `active` pixels in its list), then the next phase's prefix sum, slot
  // map, pixel list and (to the host) slot and pixel counts
  auto record = [&](int g, const double* Lph, int64_t active) -> int {
    AdaptPlan ap;
    ap.list = g == 1 ? nullptr : w.lst[g & 1].as<uint32_t>();
    ap.kcur = g == 1 ? nullptr : w.kl[g & 1].as<uint32_t>();
    ap.off = g == 1 ? nullptr : w.ol[g & 1].as<uint32_t>();
    ap.knext = w.knext.as<uint32_t>();
    ap.kuni = K1, ap.sub_n = 1, ap.sub_j = 0;
    ap.min_spp = prm->min_spp, ap.budget = budget, ap.phase = g, ap.kcap = kcap;
    // a phase of at least ~phase_slots slots while pixels remain: once few pixels are left,
    // their batches grow (up to the budget) instead of phases that are mostly launch tail
    ap.kmin = (int32_t)std::min<int64_t>(budget, (phase_slots + active - 1) / std::max<int64_t>(1, active));
    ap.rel = prm->rel_threshold;
    ap.margin_step = g_tune.phase_mstep >= 0 ? g_tune.phase_mstep : kAdaptMarginStep;
    ap.margin1 = g_tune.margin1 >= 0 ? g_tune.margin1 : kAdaptMargin1;
    ap.pool_w = (float)(g_tune.pool_w >= 0 ? g_tune.pool_w : kAdaptPoolW);
    ap.rv = w.rv.as<float>();
    ap.width = std::max(1, A.map.stripes ? A.map.W : A.map.w);  // (the render's own rows)
    ap.segs = !L.count ? nullptr : g == 1 ? sc->segs1.as<uint16_t>() : w.segs.as<uint16_t>();
    ap.rec_segs = A.counters + 9;
    ap.next_active = ctr + kSpreadBase;
    // (ap.next_active was zeroed with the phase's slot counter block, k_slot_block_init)
    const int64_t n = active;  // entries of the phase's list
    hipLaunchKernelGGL(k_adapt_record, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, px, Lph, n, npix, ap);
    HIPC(hipGetLastError());
    if (ap.pool_w > 0.0f) {
      hipLaunchKernelGGL(k_adapt_plan, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, px, n, npix, ap);
      HIPC(hipGetLastError());
    }
    hipLaunchKernelGGL(k_adapt_floor, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ap.knext, ap.list,
                       n, 1, 0, (const int32_t*)px.samples, budget, kcap, phase_slots,
                       (const unsigned long long*)ap.next_active, ctr + 8 * 16 + 1);
    HIPC(hipGetLastError());
    HIPC(rtxscan::exclusive_scan_packed(ap.knext, w.pk.as<uint64_t>(), n, w.scan_tmp.p, w.scan_tmp.n, s));
    const AdaptList next{w.lst[(g + 1) & 1].as<uint32_t>(), w.kl[(g + 1) & 1].as<uint32_t>(),
                         w.ol[(g + 1) & 1].as<uint32_t>()};
    hipLaunchKernelGGL(k_adapt_expand, dim3((unsigned)((n + kExpandPix - 1) / kExpandPix)), dim3(kBlock), 0, s,
                       (const uint32_t*)ap.knext, (const unsigned long long*)w.pk.as<unsigned long long>(), ap.list, n,
                       1, 0, (const int32_t*)px.samples, w.smap.as<uint2>(), next, ctr + 8 * 16);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(w.total_h.p, ctr + 8 * 16, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(w.ev, s));
    return RTX_OK;
  };
  // one persistent launch of a phase; debug: its time and segments on stderr
  // uniform: the launch's slot count (no slot map: uniform groups); 0: the slot map's, from k_adapt_expand
  auto launch = [&](int g, const Launch& Lg, const RenderArgs& Ag, uint16_t* segs, int64_t pixels, uint64_t nslots,
                    uint64_t uniform = 0) -> int {
    unsigned long long seg0 = 0;
    hipLaunchKernelGGL(k_slot_block_init, dim3(1), dim3(8 * 16), 0, s, ctr, uniform ? 1 : 0,
                       (unsigned long long)uniform, 0ull);
    HIPC(hipGetLastError());
    if (debug) {
      HIPC(hipStreamSynchronize(s));
      HIPC(hipMemcpy(&seg0, A.counters, sizeof seg0, hipMemcpyDeviceToHost));
      HIPC(hipEventRecord(sc->ev[2], s));
    }
    int rc2;
    if (debug) HIPC(hipMemsetAsync(A.counters + 13, 0, 5 * sizeof(unsigned long long), s));  // (the timeline)
    if ((rc2 = mark(s))) return rc2;
    if (L.count && (rc2 = set_segbuf(ctr, segs, s))) return rc2;
    if ((rc2 = trace(g, Lg, Ag, ctr, nslots))) return rc2;
    L.build = Lg.build;  // (the stats report the instantiation launched last)
    if ((rc2 = mark(s))) return rc2;
    hot_launches++;
    if (debug) {
      HIPC(hipEventRecord(sc->ev[3], s));
      HIPC(hipEventSynchronize(sc->ev[3]));
      float ms = 0;
      unsigned long long seg1 = 0;
      HIPC(hipEventElapsedTime(&ms, sc->ev[2], sc->ev[3]));
      HIPC(hipMemcpy(&seg1, A.counters, sizeof seg1, hipMemcpyDeviceToHost));
      unsigned long long tt[18] = {};
      HIPC(hipMemcpy(tt, A.counters, sizeof tt, hipMemcpyDeviceToHost));
      if (tt[13]) {  // counting build: the launch's timeline (us from the first block's start)
        const double t0 = (double)~tt[13];
        auto us = [&](unsigned long long v) { return ((double)v - t0) / 100.0; };
        fprintf(stderr, "rtx adaptive: phase %d timeline: slots used up %.1f .. %.1f us, waves end %.1f .. %.1f us\n",
                g, us(~tt[15]), us(tt[14]), us(~tt[17]), us(tt[16]));
      }
      fprintf(stderr, "rtx adaptive: phase %d: %lld pixels, launch %.3f ms, %llu segments (%.0f Mseg/s)\n", g,
              (long long)pixels, ms, seg1 - seg0, (double)(seg1 - seg0) / (ms * 1e3));
    }
    return RTX_OK;
  };
  // phase 1: min_spp samples of every pixel, one uniform launch over the whole render (the
  // scene's radiance buffer)
  if ((rc = sc->lbuf.reserve((size_t)npix * K1 * 3 * sizeof(double)))) return rc;
  if (L.count && (rc = sc->segs1.reserve((size_t)npix * K1 * sizeof(uint16_t)))) return rc;
  RenderArgs A1 = A;
  A1.L = sc->lbuf.as<double>();
  A1.conv = nullptr;
  A1.K = K1, A1.s0 = 0, A1.fK = make_fastdiv((uint32_t)K1);
  // the phase kernel without a slot map (uniform groups: slot p * K1 + k), for its block-shared
  // chunks: the first pass ends as the phases do, its last slots traced by whole blocks
  Launch L1 = L;
  const bool first_map1 = (g_tune.first_map >= 0 ? g_tune.first_map : kFirstPassMap) == 1;
  if (first_map1) L1.map = 1;
  const uint64_t nslots1 = (uint64_t)npix * (uint64_t)K1;
  if ((rc = launch(1, L1, A1, sc->segs1.as<uint16_t>(), npix, nslots1, first_map1 ? nslots1 : 0))) return rc;
  if ((rc = record(1, sc->lbuf.as<double>(), npix))) return rc;
  RenderArgs Ag = A;
  Ag.L = w.lbuf.as<double>();
  Ag.conv = nullptr;    // only pixels still sampling have slots
  Ag.K = 1, Ag.s0 = 0, Ag.fK = make_fastdiv(1u);  // (unused: slots from the phase's slot map)
  Launch Lg = L;
  Lg.map = 1;
  for (int g = 2;; g++) {
    // this phase's slot count, computed at the end of the previous one
    HIPC(hipEventSynchronize(w.ev));
    const unsigned long long nsl = ((const volatile unsigned long long*)w.total_h.p)[0];
    const int64_t active = (int64_t)((const volatile unsigned long long*)w.total_h.p)[1];
    if (nsl == 0) break;
    // the output once few pixels are left: every other pixel is final (phase g's list holds the
    // rest, and later phases' lists are subsets of it)
    if ((rc = early(g, active, w.lst[g & 1].as<uint32_t>()))) return rc;
    if ((rc = launch(g, Lg, Ag, w.segs.as<uint16_t>(), active, nsl))) return rc;
    if ((rc = record(g, Ag.L, active))) return rc;
  }
  return RTX_OK;
}

// How one uniform group of radiance records (L: npix x K records, pixel-major) enters the pixel
// statistics: render_device_impl's launches after each group, shared with the test hook
// rtx_internal_accumulate_groups.
//   kAccRecord      RecordSample + IsConverged in sample order (k_accumulate; adaptive 0: no test)
//   kAccSum         fixed spp (RecordSample's in-order sum, or the megakernel's DefaultSampler):
//                   only sum / (float)samples reaches the output, and the in-order sum is the
//                   same as RecordSample's; the Welford mean / M2 (three divisions per sample)
//                   only feed IsConverged, which adaptive sampling alone consults.  `first`: the
//                   group starts the sums; out.resolve >= 0 (the last group): the resolved output
//                   instead of the running sums, in `bands` bands of the pixels whose edges are
//                   multiples of `align` (after_band(b, q0, q1) follows each band's launch)
//   kAccMkAdaptive  the megakernel's AdaptiveSampler(min_spp, spp, rel)
enum AccKind { kAccRecord = 0, kAccSum = 1, kAccMkAdaptive = 2 };
struct GroupAcc {
  AccKind kind;
  int adaptive, min_spp, spp;
  double rel;
  bool first = false;
  AccOut out{nullptr, nullptr, -1, 0};
  int bands = 1;
  int64_t align = 1;
};
template <class AfterBand>
int accumulate_group(hipStream_t s, const PixelSoA& px, const double* L, int64_t npix, int K, const GroupAcc& ga,
                     AfterBand after_band) {
  const int pix_blocks = (int)((npix + kBlock - 1) / kBlock);
  if (ga.kind == kAccMkAdaptive)
    hipLaunchKernelGGL(k_accumulate_mk_adaptive, dim3(pix_blocks), dim3(kBlock), 0, s, px, L, npix, K, ga.min_spp,
                       ga.spp, ga.rel);
  else if (ga.kind == kAccSum) {
    AccOut out = ga.out;
    out.spp = ga.spp;
    const int nb = std::max(1, ga.bands);
    const int64_t align = std::max<int64_t>(1, ga.align);
    const int64_t units = (npix + align - 1) / align;
    int rc;
    for (int b = 0; b < nb; b++) {
      const int64_t q0 = std::min<int64_t>(npix, units * b / nb * align);
      const int64_t q1 = std::min<int64_t>(npix, units * (b + 1) / nb * align);
      if (q1 <= q0) continue;
      hipLaunchKernelGGL(k_accumulate_sum, dim3((unsigned)((q1 - q0 + kAccPix - 1) / kAccPix)), dim3(kAccWave), 0, s,
                         px, L, npix, K, q0, q1, ga.first ? 1 : 0, out);
      HIPC(hipGetLastError());
      if ((rc = after_band(b, q0, q1))) return rc;
    }
  } else
    hipLaunchKernelGGL(k_accumulate, dim3(pix_blocks), dim3(kBlock), 0, s, px, L, npix, K, ga.adaptive, ga.min_spp,
                       ga.rel);
  HIPC(hipGetLastError());
  return RTX_OK;
}

}  // namespace

extern "C" {

int rtx_abi_version(void) { return RTX_ABI_VERSION; }
const char* rtx_last_error(void) { return g_err.c_str(); }
void rtx_internal_set_error(const char* msg) { g_err = msg ? msg : ""; }

int rtx_device_count(int* n) {
  if (!n) return fail(RTX_ERR_INVALID, "n is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return fail(RTX_ERR_NODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *n = c;
  return RTX_OK;
}

int rtx_scene_create(int device, const rtx_scene_desc* d, rtx_scene** out) {
  if (!d || !out) return fail(RTX_ERR_INVALID, "NULL argument");
  *out = nullptr;
  // 1. the host's work (rtx_scene_plan.cc): checks, trees, tables, flags.  The plan outlives the
  // uploads below (and the scene, should one of them fail: ~rtx_scene waits for the stream)
  rtxplan::ScenePlan plan;
  if (const char* why = rtxplan::plan_scene(d, plan)) return fail(RTX_ERR_INVALID, why);
  // 2. the device, its stream and events
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RTX_ERR_NODEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(RTX_ERR_INVALID, "device out of range");
  auto sc = std::make_unique<rtx_scene>();
  sc->device = device;
  HIPC(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, device));
  sc->cus = prop.multiProcessorCount;
  HIPC(hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking));
  for (auto& e : sc->ev) HIPC(hipEventCreate(&e));
  hipStream_t s = sc->stream;
  // 3. the uploads, DScene's pointers, one wait
  const rtxplan::FastPlan& fp = plan.fast;
  int rc;
  if (plan.has_tris && (rc = upload(sc->tri_n, plan.tri_n.data(), plan.tri_n.size(), s))) return rc;
  if ((rc = upload(sc->prims, plan.prims.data(), plan.prims.size(), s))) return rc;
  if ((rc = upload(sc->mats, plan.mats.data(), plan.mats.size(), s))) return rc;
  if ((rc = upload(sc->texs, d->textures, d->n_textures, s))) return rc;
  std::vector<DImage> imgs(d->n_images);
  sc->texels.resize(d->n_images);
  for (int32_t i = 0; i < d->n_images; i++) {
    const rtx_image& im = d->images[i];
    imgs[i].w = im.width, imgs[i].h = im.height, imgs[i].texels = nullptr;
    if (im.width > 0 && im.height > 0 && im.texels) {
      if ((rc = upload(sc->texels[i], im.texels, (size_t)im.width * im.height * 3, s))) return rc;
      imgs[i].texels = sc->texels[i].as<uint8_t>();
    } else {
      imgs[i].w = imgs[i].h = 0;
    }
  }
  if ((rc = upload(sc->images, imgs.data(), imgs.size(), s))) return rc;
  sc->n_nodes = d->n_nodes;
  sc->stack_parity = fp.stack_parity, sc->stack_fast = fp.stack_fast;
  sc->fast_need = fp.fast_need, sc->n_f4 = fp.f4.size(), sc->fast_ok = fp.fast_ok;
  sc->n_materials = d->n_materials;
  if (sc->n_nodes > 0) {
    if ((rc = upload(sc->nodes, d->nodes, d->n_nodes, s))) return rc;
    if (fp.fast_ok && (rc = upload(sc->fnodes, fp.f4.data(), fp.f4.size(), s))) return rc;
    if ((rc = upload(sc->ref_box, plan.ref_box.data(), plan.ref_box.size(), s))) return rc;
    if ((rc = upload(sc->fast_box, plan.fast_box.data(), plan.fast_box.size(), s))) return rc;
    if ((rc = upload(sc->node_order, plan.node_order.data(), plan.node_order.size(), s))) return rc;
    if (fp.fast_ok && (rc = upload(sc->f4_order, plan.f4_order.data(), plan.f4_order.size(), s))) return rc;
  }
  sc->kinds = std::move(plan.kinds);
  sc->node_lvl = std::move(plan.node_lvl), sc->f4_lvl = std::move(plan.f4_lvl);
  sc->emit_idx = std::move(plan.emit_idx);
  if (!sc->emit_idx.empty()) {
    if ((rc = upload(sc->emit_prim, sc->emit_idx.data(), sc->emit_idx.size(), s))) return rc;
    if ((rc = sc->emit_cum.reserve(sc->emit_idx.size() * sizeof(double)))) return rc;
    if ((rc = emitters_rebuild(sc.get(), s))) return rc;
  }
  DScene& S = sc->S;
  S.nodes = sc->nodes.as<rtx_bvh_node>();
  S.prims = sc->prims.as<rtx_prim>();
  S.tri_n = sc->tri_n.p ? sc->tri_n.as<double>() : nullptr;
  S.mats = sc->mats.as<rtx_material>();
  S.texs = sc->texs.as<rtx_texture>();
  S.images = sc->images.as<DImage>();
  S.f4nodes = (fp.f4.empty() || !sc->fast_ok) ? nullptr : sc->fnodes.as<FastNode>();
  S.n_prims = plan.n_prims;
  S.use_bvh = plan.use_bvh, S.froot_leaf = plan.froot_leaf, S.froot_count = plan.froot_count;
  S.has_tris = plan.has_tris, S.tree_kind = plan.tree_kind;
  S.all_lambertian = plan.all_lambertian, S.no_textures = plan.no_textures;
  S.n_global = plan.n_global, S.global[0] = plan.global[0], S.global[1] = plan.global[1];
  HIPC(hipStreamSynchronize(s));
  *out = sc.release();
  return RTX_OK;
}

int rtx_scene_destroy(rtx_scene* s) {
  delete s;
  return RTX_OK;
}

// ---- in-place updates ---------------------------------------------------------
}  // extern "C"
namespace {
int update_range_ok(const rtx_scene* sc, int64_t first, int64_t count) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (first < 0 || count < 0 || first > sc->S.n_prims || count > sc->S.n_prims - first)
    return fail(RTX_ERR_INVALID, "primitive range outside the scene");
  return RTX_OK;
}
// Rewrite the records from one source (rtxrefit::UpdateArgs) and refit both trees, lowest height
// first, all on `s`.  The range was checked by the caller.
int update_and_refit(rtx_scene* sc, int64_t first, int64_t count, const rtx_prim* d_src, const double* d_g,
                     hipStream_t s) {
  rtxrefit::UpdateArgs a{};
  a.prims = sc->prims.as<rtx_prim>();
  a.tri_n = sc->tri_n.p ? sc->tri_n.as<double>() : nullptr;
  a.ref_box = sc->n_nodes > 0 ? sc->ref_box.as<double>() : nullptr;
  a.fast_box = sc->n_nodes > 0 ? sc->fast_box.as<float>() : nullptr;
  a.first = first, a.count = count, a.src = d_src, a.src_g = d_g;
  // a rewritten global is no longer known to be a plain sphere, nor is its g[4] its radius squared
  for (int k = 0; k < (sc->S.n_global & 3); k++)
    if (sc->S.global[k] >= first && sc->S.global[k] < first + count) sc->S.n_global &= 3;
  HIPC(rtxrefit::update_prims(a, s));
  for (size_t k = 0; k + 1 < sc->node_lvl.size(); k++)
    HIPC(rtxrefit::refit_nodes(sc->nodes.as<rtx_bvh_node>(), sc->ref_box.as<double>(),
                               sc->node_order.as<uint32_t>() + sc->node_lvl[k], sc->node_lvl[k + 1] - sc->node_lvl[k], s));
  for (size_t k = 0; k + 1 < sc->f4_lvl.size(); k++)
    HIPC(rtxrefit::refit_f4(sc->fnodes.as<F4Node>(), sc->fast_box.as<float>(),
                            sc->f4_order.as<uint32_t>() + sc->f4_lvl[k], sc->f4_lvl[k + 1] - sc->f4_lvl[k], s));
  int rc;
  if ((rc = emitters_rebuild(sc, s))) return rc;  // the emitters' areas follow the new geometry
  sc->epoch++;
  return RTX_OK;
}
}  // namespace
extern "C" {

int rtx_scene_update_prims(rtx_scene* sc, int64_t first, int64_t count, const rtx_prim* prims) {
  int rc;
  if ((rc = update_range_ok(sc, first, count))) return rc;
  if (count == 0) return RTX_OK;
  if (!prims) return fail(RTX_ERR_INVALID, "prims is NULL");
  for (int64_t i = 0; i < count; i++) {
    const rtx_prim& p = prims[i];
    if (p.kind != sc->kinds[(size_t)(first + i)]) return fail(RTX_ERR_INVALID, "an update may not change a primitive's kind");
    if (p.material < 0 || p.material >= sc->n_materials) return fail(RTX_ERR_INVALID, "primitive material out of range");
    const int used = p.kind == RTX_PRIM_SPHERE ? 4 : (p.kind == RTX_PRIM_TRIANGLE ? 9 : 5);
    for (int k = 0; k < used; k++)
      if (!std::isfinite(p.g[k])) return fail(RTX_ERR_INVALID, "primitive geometry is not finite");
  }
  HIPC(hipSetDevice(sc->device));
  const size_t bytes = (size_t)count * sizeof(rtx_prim);
  if ((rc = sc->upd_host.reserve(bytes))) return rc;
  if ((rc = sc->upd_stage.reserve(bytes))) return rc;
  std::memcpy(sc->upd_host.p, prims, bytes);
  HIPC(hipMemcpyAsync(sc->upd_stage.p, sc->upd_host.p, bytes, hipMemcpyHostToDevice, sc->stream));
  if ((rc = update_and_refit(sc, first, count, sc->upd_stage.as<rtx_prim>(), nullptr, sc->stream))) return rc;
  HIPC(hipStreamSynchronize(sc->stream));  // the staging buffers are free again; a kernel failure shows here
  return RTX_OK;
}

int rtx_scene_update_geometry_device(rtx_scene* sc, int64_t first, int64_t count, const double* d_g, void* stream) {
  int rc;
  if ((rc = update_range_ok(sc, first, count))) return rc;
  if (count == 0) return RTX_OK;
  if (!d_g) return fail(RTX_ERR_INVALID, "d_g is NULL");
  HIPC(hipSetDevice(sc->device));
  return update_and_refit(sc, first, count, nullptr, d_g, stream ? (hipStream_t)stream : sc->stream);
}

int rtx_scene_epoch(const rtx_scene* sc, int64_t* epoch) {
  if (!sc || !epoch) return fail(RTX_ERR_INVALID, "NULL argument");
  *epoch = sc->epoch;
  return RTX_OK;
}

// Test hook (not in rtx.h): the device's reference-layout nodes (64 bytes each, at most
// nodes_cap) and fast nodes (128 bytes each, at most f4_cap; none when the scene has no fast
// tree) copied back to the host, after everything queued on the scene's stream.
int rtx_internal_scene_trees(rtx_scene* sc, void* nodes_out, int64_t nodes_cap, void* f4_out, int64_t f4_cap) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  HIPC(hipSetDevice(sc->device));
  const int64_t nn = std::min<int64_t>(std::max<int64_t>(0, nodes_cap), sc->n_nodes);
  const int64_t nf = std::min<int64_t>(std::max<int64_t>(0, f4_cap), sc->fast_ok ? (int64_t)sc->n_f4 : 0);
  if (nodes_out && nn)
    HIPC(hipMemcpyAsync(nodes_out, sc->nodes.p, (size_t)nn * sizeof(rtx_bvh_node), hipMemcpyDeviceToHost, sc->stream));
  if (f4_out && nf)
    HIPC(hipMemcpyAsync(f4_out, sc->fnodes.p, (size_t)nf * sizeof(F4Node), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

// Test hook (not in rtx.h): the primary rays the render kernels generate for the pixel subset of
// prm (its subset and seed are read), samples [first_sample, first_sample + spp) of each pixel:
// npix x spp x 6 doubles (origin, direction), pixel major, from get_ray with
// make_rng(seed, global pixel, sample, 0) as k_wf_generate calls it.
extern "C" int rtx_internal_camera_rays(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm,
                                        int32_t first_sample, int32_t spp, double* out) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!cam || !prm) return fail(RTX_ERR_INVALID, "NULL argument");
  if (!out) return fail(RTX_ERR_INVALID, "NULL buffer");
  if (spp < 1) return fail(RTX_ERR_INVALID, "camera rays: spp must be at least 1");
  if (first_sample < 0 || first_sample > 0x7FFFFFFF - spp)
    return fail(RTX_ERR_INVALID, "camera rays: first_sample must be >= 0 and first_sample + spp fit int32");
  PixelMap map;
  std::string err;
  const int64_t npix = subset_pixels(cam, prm, map, err);
  if (npix < 0) return fail(RTX_ERR_INVALID, err);
  if (npix == 0) return RTX_OK;
  if (npix * (int64_t)spp > kRadianceSlotsMax) return fail(RTX_ERR_INVALID, "camera rays: too many rays for one call");
  HIPC(hipSetDevice(sc->device));
  const uint32_t nslots = (uint32_t)(npix * spp);
  const size_t bytes = (size_t)nslots * 6 * sizeof(double);
  int rc;
  if ((rc = sc->rays.reserve(bytes))) return rc;
  hipLaunchKernelGGL(k_camera_rays, dim3((nslots + kBlock - 1) / kBlock), dim3(kBlock), 0, sc->stream, *cam, map, nslots,
                     (uint32_t)spp, prm->seed, first_sample, sc->rays.as<double>());
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(out, sc->rays.p, bytes, hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

// Camera::Initialize (camera.h:100-131), same operation order as the reference.
int rtx_camera_init(const rtx_camera_config* c, rtx_camera* o) {
  if (!c || !o) return fail(RTX_ERR_INVALID, "NULL argument");
  if (c->image_width <= 0 || !(c->aspect_ratio > 0)) return fail(RTX_ERR_INVALID, "bad image width / aspect ratio");
  const double kPiH = 3.14159265358979323846;
  auto sub = [](const double* a, const double* b, double* r) { for (int i = 0; i < 3; i++) r[i] = a[i] - b[i]; };
  auto scale = [](double t, const double* a, double* r) { for (int i = 0; i < 3; i++) r[i] = t * a[i]; };
  auto norm = [&](const double* a, double* r) {
    double l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (l == 0.0) { r[0] = r[1] = r[2] = 0; return; }
    scale(1.0 / l, a, r);
  };
  auto cross = [](const double* u, const double* v, double* r) {
    r[0] = u[1] * v[2] - u[2] * v[1];
    r[1] = u[2] * v[0] - u[0] * v[2];
    r[2] = u[0] * v[1] - u[1] * v[0];
  };
  std::memset(o, 0, sizeof *o);
  int H = int(c->image_width / c->aspect_ratio);
  H = H < 1 ? 1 : H;
  o->image_width = c->image_width, o->image_height = H;
  for (int i = 0; i < 3; i++) o->center[i] = c->lookfrom[i];
  double theta = c->vfov * (kPiH / 180.0);
  double h = std::tan(theta / 2);
  double vh = 2 * h * c->focus_dist;
  double vw = vh * (double(c->image_width) / H);
  double t[3], vu[3], vv[3], negv[3];
  sub(c->lookfrom, c->lookat, t);
  norm(t, o->w);
  cross(c->vup, o->w, t);
  norm(t, o->u);
  cross(o->w, o->u, o->v);
  scale(vw, o->u, vu);
  for (int i = 0; i < 3; i++) negv[i] = -o->v[i];
  scale(vh, negv, vv);
  scale(1.0 / (double)c->image_width, vu, o->pixel_delta_u);
  scale(1.0 / (double)H, vv, o->pixel_delta_v);
  double fw[3], hu[3], hv[3], ul[3], sdd[3], hd[3];
  scale(c->focus_dist, o->w, fw);
  scale(1.0 / 2.0, vu, hu);
  scale(1.0 / 2.0, vv, hv);
  for (int i = 0; i < 3; i++) ul[i] = ((o->center[i] - fw[i]) - hu[i]) - hv[i];
  for (int i = 0; i < 3; i++) sdd[i] = o->pixel_delta_u[i] + o->pixel_delta_v[i];
  scale(0.5, sdd, hd);
  for (int i = 0; i < 3; i++) o->pixel00[i] = ul[i] + hd[i];
  double rad = c->focus_dist * std::tan((c->defocus_angle / 2) * (kPiH / 180.0));
  scale(rad, o->u, o->defocus_disk_u);
  scale(rad, o->v, o->defocus_disk_v);
  o->defocus_angle = c->defocus_angle;
  return RTX_OK;
}

int64_t rtx_render_pixel_count(const rtx_camera* cam, const rtx_render_params* p) {
  if (!cam || !p) return fail(RTX_ERR_INVALID, "NULL argument");
  PixelMap m;
  std::string err;
  int64_t n = subset_pixels(cam, p, m, err);
  if (n < 0) return fail(RTX_ERR_INVALID, err);
  return n;
}

// Whose pixel state a render advances and from which sample.  rtx_render*: the scene's own
// px_* buffers, started here, samples [0, spp), resolved into the caller's buffers (no FilmRun).
// A film: its own state, holding samples [0, done) already; the render adds [done, spp) and
// leaves the running sums in place (the film resolves on demand, k_film_resolve).
struct FilmRun {
  PixelSoA px;
  int32_t done;
};
static int render_device_impl(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* d_rgb,
                              int32_t* d_spp, rtx_stats* stats, void* stream, const BandSink* sink,
                              const FilmRun* film = nullptr);
// Whether render_device_impl hands a render's output to a BandSink: fixed-spp renders
// (RecordSample's in-order sum or the megakernel's DefaultSampler) with samples to trace.
static bool sum_path_of(const rtx_render_params* prm) {
  const bool mk_adaptive = prm->adaptive && prm->mode == RTX_MODE_MEGAKERNEL;
  return !mk_adaptive && (prm->mode == RTX_MODE_MEGAKERNEL || !prm->adaptive) && prm->spp > 0;
}

int rtx_render_device(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* d_rgb,
                      int32_t* d_spp, rtx_stats* stats, void* stream) {
  return render_device_impl(sc, cam, prm, d_rgb, d_spp, stats, stream, nullptr);
}

static int render_device_impl(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* d_rgb,
                              int32_t* d_spp, rtx_stats* stats, void* stream, const BandSink* sink,
                              const FilmRun* film) {
  if (!sc || !cam || !prm || (!d_rgb && !film)) return fail(RTX_ERR_INVALID, "NULL argument");
  if (prm->spp < 0 || prm->max_depth < 0) return fail(RTX_ERR_INVALID, "negative spp / max_depth");
  if (prm->mode < RTX_MODE_WAVEFRONT || prm->mode > RTX_MODE_MEGAKERNEL) return fail(RTX_ERR_INVALID, "bad mode");
  // MegaKernel + adaptive = AdaptiveSampler(min_spp, spp, rel_threshold): up to spp + 1 samples
  const bool mk_adaptive = prm->adaptive && prm->mode == RTX_MODE_MEGAKERNEL;
  if (mk_adaptive && prm->spp >= 0x7FFFFFFF) return fail(RTX_ERR_INVALID, "spp too large");
  const int budget = mk_adaptive ? prm->spp + 1 : prm->spp;
  // the first sample to trace: 0, or the samples a film holds already
  const int s_begin = film ? film->done : 0;
  if (film && (mk_adaptive || s_begin < 0 || s_begin > budget)) return fail(RTX_ERR_INVALID, "bad film sample range");
  PixelMap map;
  std::string err;
  const int64_t npix = subset_pixels(cam, prm, map, err);
  if (npix < 0) return fail(RTX_ERR_INVALID, err);
  HIPC(hipSetDevice(sc->device));
  hipStream_t s = stream ? (hipStream_t)stream : sc->stream;
  const bool fast = prm->precision == RTX_PREC_FAST && sc->fast_ok;
  Launch L{sc, s, fast ? sc->stack_fast : sc->stack_parity, fast, (prm->flags & RTX_FLAG_COUNT) != 0};
  L.generic = (prm->flags & RTX_FLAG_GENERIC) != 0;
  if (fast && prm->mode == RTX_MODE_PERSISTENT) {
    bool park;
    if (prm->flags & RTX_FLAG_PARK) park = true;
    else if (prm->flags & RTX_FLAG_NO_PARK) park = false;
    else {
      int rc;
      if (sc->park < 0 && (rc = time_park_schedule(sc, cam, prm, s))) return rc;
      park = sc->park == 1;
    }
    // the speculative walk keeps 16-bit node indices on its stack: larger trees (and renders
    // that ask for it) get the leaf-step walk
    const bool spec = sc->n_f4 <= kSpecMaxNodes && !(prm->flags & RTX_FLAG_LEAF_STEP);
    L.park = park ? (spec ? 2 : 1) : 0;
  }

  // the reference's default sampling (adaptive) on the persistent kernel: in phases
  // (render_adaptive); an explicit samples_per_group keeps uniform groups
  const bool phased = prm->mode == RTX_MODE_PERSISTENT && prm->adaptive && !mk_adaptive &&
                      prm->samples_per_group <= 0 && budget > 0 && npix > 0 && s_begin == 0;
  // One allowance (slot_allowance) for all of a scene's slot buffers: the radiance buffer of
  // uniform groups and of the adaptive first pass (lbuf), the wavefront's path queues, the
  // adaptive phases' workspace (aw).  A render keeps the other kinds' buffers as long as they
  // and what it needs itself fit in the allowance, and releases them only when they do not:
  // every release and reallocation synchronises the device, and frames that alternate kinds
  // (the bench's fixed-spp line, its adaptive leg, the CPU check) would pay it every time.
  // A phased render's first pass runs in the scene's radiance buffer (lbuf) at npix x min_spp
  // slots: whatever a fixed-spp frame left there beyond that is kept like another kind's buffer.
  double other = 0.0;  // bytes of other kinds kept (phased: and lbuf beyond the first pass)
  {
    const bool wf = prm->mode == RTX_MODE_WAVEFRONT;
    const double allow = slot_allowance(sc);
    const double per_slot = phased ? 34.0 : wf ? 24.0 + 2 * 84.0 : 24.0;  // (phases: radiance, slot map, batches)
    const double want = per_slot * (double)npix * (double)std::max(1, budget);
    const double aw_bytes = (double)sc->aw.lbuf.n + (double)sc->aw.smap.n + (double)sc->aw.segs.n;
    const double queue_bytes = (double)sc->queue[0].n + (double)sc->queue[1].n;
    const double first_bytes = phased ? adaptive_first_bytes(npix, prm, budget, L.count) : 0.0;
    const double lbuf_extra = phased ? std::max(0.0, (double)sc->lbuf.n - first_bytes) : 0.0;
    other = (phased ? lbuf_extra : aw_bytes) + (wf ? 0.0 : queue_bytes);
    if (other + std::min(want, per_slot * (double)(1ll << kSlotTargetLog2)) > allow) {
      if (!phased) sc->aw.lbuf.release(), sc->aw.smap.release(), sc->aw.segs.release();
      else if (lbuf_extra > 0.0) sc->lbuf.release();  // (render_adaptive reserves the first pass's size)
      if (!wf)
        for (auto& q : sc->queue) q.release();
      other = 0.0;
    }
  }

  // samples in flight per pixel (group size K)
  int K = prm->samples_per_group;
  if (K <= 0) {
    // slots in flight: each persistent launch ends in a tail of draining lanes, so fewer,
    // larger groups pay it less often (Lbuf = 24 B per slot); the wavefront's two queues cost
    // 84 B per slot each and keep the smaller target
    const int64_t target =
        prm->mode == RTX_MODE_WAVEFRONT
            ? slot_target(sc, 3 * sizeof(double) + 2 * (9 * sizeof(double) + 3 * sizeof(uint32_t)), 1ll << 25, other)
            : slot_target(sc, 3 * sizeof(double), 1ll << kSlotTargetLog2, other);
    K = (int)std::max<int64_t>(1, std::min<int64_t>(budget > s_begin ? budget - s_begin : 1,
                                                    target / std::max<int64_t>(1, npix)));
  }
  K = std::max(1, std::min(K, std::max(1, budget - s_begin)));
  if ((int64_t)npix * K > 0xFFFFFFFFll) return fail(RTX_ERR_INVALID, "too many slots in one group (lower samples_per_group)");
  const int64_t nslots = npix * (int64_t)K;

  int rc;
  if (!film) {
    if ((rc = sc->px_sum.reserve(npix * 3 * sizeof(double)))) return rc;
    if ((rc = sc->px_mean.reserve(npix * 3 * sizeof(double)))) return rc;
    if ((rc = sc->px_m2.reserve(npix * 3 * sizeof(double)))) return rc;
    if ((rc = sc->px_samples.reserve(npix * sizeof(int32_t)))) return rc;
    if ((rc = sc->px_conv.reserve(npix))) return rc;
  }
  if (!phased && (rc = sc->lbuf.reserve(nslots * 3 * sizeof(double)))) return rc;
  if ((rc = sc->counters.reserve(kCounterWords * sizeof(unsigned long long)))) return rc;
  const size_t qbytes = nslots * (9 * sizeof(double) + 3 * sizeof(uint32_t));
  if (prm->mode == RTX_MODE_WAVEFRONT)
    for (auto& q : sc->queue)
      if ((rc = q.reserve(qbytes))) return rc;
  // fixed spp (RecordSample's in-order sum, or the megakernel's DefaultSampler): only the
  // running sum and count matter, and the first group starts them (k_accumulate_sum `first`)
  const bool sum_path = sum_path_of(prm);
  const PixelSoA px = film ? film->px
                           : PixelSoA{sc->px_sum.as<double>(), sc->px_mean.as<double>(), sc->px_m2.as<double>(),
                                      sc->px_samples.as<int32_t>(), sc->px_conv.as<uint8_t>()};
  {
    // the counters always; the pixel state only where the render starts it (a film that holds
    // samples keeps them)
    const int zero_px = (sum_path || s_begin > 0) ? 0 : 1;
    const int64_t n = std::max<int64_t>(zero_px ? npix : 0, kCounterWords);
    hipLaunchKernelGGL(k_frame_init, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, px, npix,
                       zero_px, sc->counters.as<unsigned long long>(), kCounterWords);
    HIPC(hipGetLastError());
    if (g_debug_host) g_t_launch = host_us();
  }
  const bool banded = sum_path && sink && npix > 0;
  const bool early_ok = phased && sink && sink->host_rgb_dev && npix > 0;
  if (banded || early_ok) {
    if (!sc->copy_stream) HIPC(hipStreamCreateWithFlags(&sc->copy_stream, hipStreamNonBlocking));
    while (sc->band_ev.size() < kBands + 1) {
      hipEvent_t e = nullptr;
      HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      sc->band_ev.push_back(e);
    }
  }
  bool resolved = false;

  unsigned long long* cnt = sc->counters.as<unsigned long long>();
  RenderArgs A;
  A.S = sc->S;
  A.cam = *cam;
  A.map = map;
  A.seed = prm->seed;
  A.npix = npix;
  A.max_depth = prm->max_depth;
  A.scatter_api = prm->mode == RTX_MODE_MEGAKERNEL;
  A.conv = prm->adaptive ? px.conv : nullptr;
  A.L = sc->lbuf.as<double>();
  A.counters = cnt;
  // the lean BVH4 walk stores at most fast_need + 1 stack slots (branchless pushes); the
  // parity walk gets its template bound (pick_stack, rtx_scene_plan.cc: reference depth + 2)
  A.stack_slots = fast ? sc->fast_need + 1 : L.stack + 1;
  // counters[8..] : queue counts (u32) for the wavefront;
  // [64 + 16 g] the slot counters of the 8 regions, 128 bytes apart
  unsigned* qcount = (unsigned*)(cnt + 8);
  unsigned long long* next_slot = cnt + 64;
  auto make_queue = [&](DevBuf& b) {
    PathQueue q;
    double* d = b.as<double>();
    q.ox = d, q.oy = d + nslots, q.oz = d + 2 * nslots, q.dx = d + 3 * nslots, q.dy = d + 4 * nslots;
    q.dz = d + 5 * nslots, q.tx = d + 6 * nslots, q.ty = d + 7 * nslots, q.tz = d + 8 * nslots;
    q.slot = (uint32_t*)(d + 9 * nslots);
    q.meta = q.slot + nslots;
    q.hit = (int32_t*)(q.meta + nslots);
    return q;
  };
  // per-launch timing of the dominant kernel (extend / persistent) with an event pool: one
  // pair per hot launch of the whole frame (grow-only pool)
  size_t evi = 0;
  const bool timed = stats != nullptr;
  double hot_ms = 0;
  uint64_t hot_launches = 0;
  if (timed) HIPC(hipEventRecord(sc->ev[0], s));
  const int pix_blocks = (int)((npix + kBlock - 1) / kBlock);
  const int wf_grid = std::max(1, std::min<int>(sc->cus * 16, (int)((nslots + kBlock - 1) / kBlock)));
  // Adaptive early output: once a phase holds at most npix / kEarlyOutDiv pixels, every other
  // pixel is final, so the whole output is resolved and copied to the host on the copy stream
  // while the remaining phases run; at the end the device writes only that phase's pixels into
  // the host framebuffer (k_patch_host).  (The copy engine does not need the CUs the phase
  // launches hold.)
  int64_t patch_n = -1;
  auto early = [&](int g, int64_t active, const uint32_t* list) -> int {
    (void)g;
    if (!early_ok || patch_n >= 0 || active * kEarlyOutDiv > npix) return RTX_OK;
    int rc2;
    if ((rc2 = sc->patch_q.reserve((size_t)std::max<int64_t>(1, active) * sizeof(uint32_t)))) return rc2;
    hipLaunchKernelGGL(k_resolve, dim3(pix_blocks), dim3(kBlock), 0, s, px, npix, 0, prm->spp, d_rgb, d_spp);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(sc->patch_q.p, list, (size_t)active * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    HIPC(hipEventRecord(sc->band_ev[0], s));
    HIPC(hipStreamWaitEvent(sc->copy_stream, sc->band_ev[0], 0));
    if ((rc2 = sink->copy(sink->ctx, 0, npix, sc->copy_stream))) return rc2;
    HIPC(hipEventRecord(sc->band_ev[1], sc->copy_stream));
    patch_n = active;
    g_early_outputs++, g_early_patched += active;
    return RTX_OK;
  };
  if (phased) {
    if ((rc = render_adaptive(sc, L, A, prm, px, budget, other, s, [&](hipStream_t st) -> int {
           if (timed) {
             hipEvent_t e = sc->pool_event(evi++);
             if (!e) return fail(RTX_ERR_HIP, "hipEventCreate failed");
             HIPC(hipEventRecord(e, st));
           }
           return RTX_OK;
         }, hot_launches, early, trace_persistent))) {
      // an error after the early output was queued: the copy into the caller's framebuffer
      // must be over before the caller gets the error (and may free or reuse the buffer)
      if (patch_n >= 0) (void)hipEventSynchronize(sc->band_ev[1]);
      return rc;
    }
    if (patch_n >= 0) {  // the early copy is done before the device patches the same framebuffer
      hipError_t e = hipStreamWaitEvent(s, sc->band_ev[1], 0);
      if (e == hipSuccess && patch_n > 0) {
        hipLaunchKernelGGL(k_patch_host, dim3((unsigned)((patch_n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, px,
                           npix, sc->patch_q.as<uint32_t>(), patch_n, map, sink->host_rgb_dev, d_rgb, d_spp);
        e = hipGetLastError();
      }
      if (e != hipSuccess) {
        (void)hipEventSynchronize(sc->band_ev[1]);
        return fail(RTX_ERR_HIP, std::string("adaptive early output: ") + hipGetErrorString(e));
      }
      resolved = true;
    }
  }
  for (int s0 = s_begin, Kc = 0; s0 < budget && !phased; s0 += Kc) {
    Kc = std::min(K, budget - s0);
    // adaptive with automatic grouping: nothing can converge before min_spp, afterwards
    // small groups limit the samples traced past a pixel's convergence point
    if (prm->adaptive && prm->samples_per_group <= 0)
      Kc = std::min(Kc, s0 < prm->min_spp ? prm->min_spp - s0 : 4);
    A.K = Kc;
    A.fK = make_fastdiv((uint32_t)Kc);
    A.s0 = s0;
    auto hot_begin = [&]() -> int {
      if (timed) {
        hipEvent_t e = sc->pool_event(evi++);
        if (!e) return fail(RTX_ERR_HIP, "hipEventCreate failed");
        HIPC(hipEventRecord(e, s));
      }
      return RTX_OK;
    };
    if (prm->mode == RTX_MODE_WAVEFRONT) {
      PathQueue q[2] = {make_queue(sc->queue[0]), make_queue(sc->queue[1])};
      HIPC(hipMemsetAsync(qcount, 0, 2 * sizeof(unsigned), s));
      hipLaunchKernelGGL(k_wf_generate, dim3(wf_grid), dim3(kBlock), 0, s, A, q[0], qcount);
      HIPC(hipGetLastError());
      for (int b = 0; b <= prm->max_depth; b++) {
        const int cur = b & 1;
        HIPC(hipMemsetAsync(qcount + (cur ^ 1), 0, sizeof(unsigned), s));
        if ((rc = hot_begin())) return rc;
        if ((rc = extend(L, A, q[cur], qcount + cur, Kc * npix))) return rc;
        if ((rc = hot_begin())) return rc;
        hipLaunchKernelGGL(k_wf_shade, dim3(wf_grid), dim3(kBlock), 0, s, A, q[cur], qcount + cur, q[cur ^ 1],
                           qcount + (cur ^ 1));
        HIPC(hipGetLastError());
        hot_launches++;
      }
    } else {
      HIPC(hipMemsetAsync(next_slot, 0, 8 * 16 * sizeof(unsigned long long), s));
      if ((rc = hot_begin())) return rc;
      rc = prm->mode == RTX_MODE_MEGAKERNEL ? persist_m<true>(L, A, next_slot) : persist_m<false>(L, A, next_slot);
      if (rc) return rc;
      if ((rc = hot_begin())) return rc;
      hot_launches++;
    }
    // fixed spp: the last group writes the resolved output itself (k_resolve's arithmetic), in
    // bands when a sink takes them
    const bool last = s0 + Kc >= budget;
    GroupAcc ga{mk_adaptive ? kAccMkAdaptive : sum_path ? kAccSum : kAccRecord, prm->adaptive, prm->min_spp, prm->spp,
                prm->rel_threshold};
    ga.first = s0 == 0;
    if (sum_path && last && !film) ga.out = AccOut{d_rgb, d_spp, prm->mode == RTX_MODE_MEGAKERNEL ? 1 : 0, prm->spp};
    if (sum_path && last && banded) ga.bands = kBands, ga.align = std::max<int64_t>(1, sink->align);
    if ((rc = accumulate_group(s, px, A.L, npix, Kc, ga, [&](int b, int64_t q0, int64_t q1) -> int {
           if (!(sum_path && last && banded)) return RTX_OK;
           HIPC(hipEventRecord(sc->band_ev[b], s));
           HIPC(hipStreamWaitEvent(sc->copy_stream, sc->band_ev[b], 0));
           return sink->copy(sink->ctx, q0, q1, sc->copy_stream);
         })))
      return rc;
    if (sum_path) resolved = last;
  }
  if (!resolved && !film) {
    hipLaunchKernelGGL(k_resolve, dim3(pix_blocks), dim3(kBlock), 0, s, px, npix,
                       prm->mode == RTX_MODE_MEGAKERNEL ? (mk_adaptive ? 2 : 1) : 0, prm->spp, d_rgb, d_spp);
    HIPC(hipGetLastError());
  }
  // the render's end (rtx_stats.kernel_ms: device time of the render, its output copies not
  // included, whatever the sampling)
  if (timed) HIPC(hipEventRecord(sc->ev[1], s));
  // renders the accumulate does not band (adaptive sampling): the whole output to the sink here,
  // on the stream before the event the host waits on, so one host wait covers the frame and its copy
  if (sink && !banded && npix > 0 && patch_n < 0) {
    if ((rc = sink->copy(sink->ctx, 0, npix, s))) return rc;
  }
  if (timed) {  // the statistics come back with the frame: one wait, no blocking copy after it
    if ((rc = sc->counters_h.reserve(24 * sizeof(unsigned long long)))) return rc;
    HIPC(hipMemcpyAsync(sc->counters_h.p, cnt, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(sc->ev[4], s));
  }
  if (banded) {  // the caller's stream owns the output again once the band copies are done
    HIPC(hipEventRecord(sc->band_ev.back(), sc->copy_stream));
    HIPC(hipStreamWaitEvent(s, sc->band_ev.back(), 0));
  }
  if (timed) {
    if (g_debug_host) g_t_sync0 = host_us();
    HIPC(hipEventSynchronize(sc->ev[4]));
    if (g_debug_host) g_t_sync1 = host_us();
    float ms = 0;
    HIPC(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1]));
    // the hot launches' event pairs are read only now: no host wait inside the frame, so the
    // accumulate / resolve launches are queued while the hot kernel still runs
    if ((rc = sc->pool_pairs_ms(evi, hot_ms))) return rc;
    unsigned long long h[24];
    std::memcpy(h, sc->counters_h.p, sizeof h);
    static const bool drain_debug = std::getenv("RTX_DEBUG_DRAIN") != nullptr;
    static const bool region_debug = std::getenv("RTX_DEBUG_REGIONS") != nullptr;
    if (region_debug && (h[18] | h[19] | h[20])) {  // counting builds: the persistent loop's regions
      const double tot = (double)(h[18] + h[19] + h[20]);
      fprintf(stderr,
              "rtx regions: wave cycles refill %.4f walk %.4f shade %.4f of %.4g (leaf rounds of the speculative "
              "walk %.4f); shading rounds %llu, lanes per shading round %.2f; segments %llu\n",
              h[18] / tot, h[19] / tot, h[20] / tot, tot, h[23] / tot, (unsigned long long)h[21],
              h[21] ? (double)h[22] / h[21] : 0.0, (unsigned long long)h[0]);
    }
    if (drain_debug && h[13] && !phased) {  // counting builds: the (last) launch's timeline
      const double t0 = (double)~h[13];
      auto us = [&](unsigned long long v) { return ((double)v - t0) / 100.0; };
      fprintf(stderr, "rtx frame timeline: slots used up %.1f .. %.1f us, waves end %.1f .. %.1f us (%lld segments)\n",
              us(~h[15]), us(h[14]), us(~h[17]), us(h[16]), (long long)h[0]);
    }
    stats->wave_rounds = h[10];
    stats->wave_rounds_idle = h[11];
    stats->wave_lanes_live = h[12];
    stats->rays_total = h[0];
    stats->parked = L.park ? 1 : 0;
    stats->rays_primary = h[1];
    stats->paths = h[1];
    stats->kernel_ms = ms;
    stats->hot_kernel_ms = hot_ms;
    stats->hot_launches = hot_launches;
    stats->node_visits = h[2];
    stats->prim_tests = h[3];
    stats->wave_node_iters = h[4];
    stats->wave_prim_iters = h[5];
    stats->tri_tests = h[6];
    stats->sphere_tests = h[7];
    stats->build = prm->mode == RTX_MODE_WAVEFRONT ? 0 : L.build;
    stats->node_bytes = L.fast ? sizeof(F4Node) : sizeof(rtx_bvh_node);  // (the byte model's 4 x 32 B boxes; a QNode is 64 B)
    // segments of the recorded samples: counted per slot by the counting build in adaptive
    // phases (k_adapt_record); every sample is recorded at fixed spp; unknown otherwise
    stats->rays_recorded = !L.count ? 0 : phased ? h[9] : (prm->adaptive ? 0 : h[0]);
  }
  return RTX_OK;
}

int rtx_render(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* rgb, int32_t* spp,
               rtx_stats* stats) {
  if (!sc || !cam || !prm || !rgb) return fail(RTX_ERR_INVALID, "NULL argument");
  PixelMap map;
  std::string err;
  const int64_t npix = subset_pixels(cam, prm, map, err);
  if (npix < 0) return fail(RTX_ERR_INVALID, err);
  HIPC(hipSetDevice(sc->device));
  int rc;
  if ((rc = sc->out_rgb.reserve(std::max<int64_t>(1, npix) * 3 * sizeof(double)))) return rc;
  if ((rc = sc->out_spp.reserve(std::max<int64_t>(1, npix) * sizeof(int32_t)))) return rc;
  if ((rc = rtx_render_device(sc, cam, prm, sc->out_rgb.as<double>(), sc->out_spp.as<int32_t>(), stats, sc->stream)))
    return rc;
  HIPC(hipMemcpyAsync(rgb, sc->out_rgb.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
  if (spp) HIPC(hipMemcpyAsync(spp, sc->out_spp.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

// ---- one frame over several devices (wavefront.cc:228-241's one framebuffer) ----
namespace {
// Device k renders stripe (first + k) of `count` interleaved stripes; its packed stripe rows
// come back over one D2H copy (pinned staging, or a 2D copy straight into a pinned caller
// buffer) and are placed at their rows of the whole-frame buffers.
int render_stripes_to_host(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* base, int stripe,
                           double* out_rgb, int32_t* out_spp, rtx_stats* st) {
  const double t_in = g_debug_host ? host_us() : 0.0;
  rtx_render_params q = *base;
  q.stripe_index = stripe;
  q.x0 = q.y0 = q.w = q.h = 0;
  PixelMap map;
  std::string err;
  const int64_t npix = subset_pixels(cam, &q, map, err);
  if (npix < 0) return fail(RTX_ERR_INVALID, err);
  HIPC(hipSetDevice(sc->device));
  int rc;
  if ((rc = sc->out_rgb.reserve(std::max<int64_t>(1, npix) * 3 * sizeof(double)))) return rc;
  if ((rc = sc->out_spp.reserve(std::max<int64_t>(1, npix) * sizeof(int32_t)))) return rc;
  const int64_t W = map.W, H = map.H, R = map.srows, N = map.scount;
  const int64_t nblk = (H + R - 1) / R;  // stripes of the image; ours: stripe, stripe + N, ...
  const size_t row_rgb = (size_t)W * 3 * sizeof(double), row_spp = (size_t)W * sizeof(int32_t);
  hipPointerAttribute_t at{};
  const bool pinned = hipPointerGetAttributes(&at, out_rgb) == hipSuccess && at.type == hipMemoryTypeHost;
  (void)hipGetLastError();  // pageable memory reports an error here on some runtimes
  const int64_t full = (H / R > stripe) ? (H / R - stripe + N - 1) / N : 0;  // our stripes with R rows
  const bool direct = pinned && full > 0;  // strided DMA straight into the caller's rows
  if (!direct && (rc = sc->stage_rgb.reserve((size_t)std::max<int64_t>(1, npix) * 3 * sizeof(double)))) return rc;
  // Packed pixels [p0, p1) of this device's rows -> host.  Band edges are whole stripes
  // (align R * W), so a band is a run of our full stripes (one strided DMA) and, in the last
  // band, the short stripe at the bottom of the image.
  struct Ctx {
    rtx_scene* sc;
    double* out_rgb;
    bool direct;
    int64_t W, R, N, stripe, full;
    size_t row_rgb;
  } ctx{sc, out_rgb, direct, W, R, N, stripe, full, row_rgb};
  auto copy = [](void* c, int64_t p0, int64_t p1, hipStream_t cs) -> int {
    const Ctx& k = *(const Ctx*)c;
    const double* src = k.sc->out_rgb.as<double>();
    if (!k.direct) {
      HIPC(hipMemcpyAsync((double*)k.sc->stage_rgb.p + 3 * p0, src + 3 * p0, (size_t)(p1 - p0) * 3 * sizeof(double),
                          hipMemcpyDeviceToHost, cs));
      return RTX_OK;
    }
    const int64_t r0 = p0 / k.W, r1 = (p1 + k.W - 1) / k.W;  // packed rows
    const int64_t k0 = r0 / k.R, k1 = std::min<int64_t>(k.full, r1 / k.R);
    if (k1 > k0)
      HIPC(hipMemcpy2DAsync(k.out_rgb + (size_t)(k.stripe + k0 * k.N) * k.R * k.W * 3, (size_t)k.N * k.R * k.row_rgb,
                            src + (size_t)k0 * k.R * k.W * 3, (size_t)k.R * k.row_rgb, (size_t)k.R * k.row_rgb,
                            (size_t)(k1 - k0), hipMemcpyDeviceToHost, cs));
    const int64_t rs = std::max<int64_t>(r0, k.full * k.R);  // rows of the short last stripe
    if (r1 > rs)
      HIPC(hipMemcpyAsync(k.out_rgb + (size_t)((k.stripe + k.full * k.N) * k.R + (rs - k.full * k.R)) * k.W * 3,
                          src + (size_t)rs * k.W * 3, (size_t)(r1 - rs) * k.row_rgb, hipMemcpyDeviceToHost, cs));
    return RTX_OK;
  };
  BandSink sink{R * W, copy, &ctx};
  if (direct) {  // adaptive renders may write their last pixels straight into the caller's pinned rows
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, out_rgb, 0) == hipSuccess) sink.host_rgb_dev = (double*)dp;
    else (void)hipGetLastError();
  }
  if ((rc = render_device_impl(sc, cam, &q, sc->out_rgb.as<double>(), sc->out_spp.as<int32_t>(), st, sc->stream,
                               &sink)))
    return rc;
  if (npix == 0) return RTX_OK;
  // (renders the accumulate does not band sent the whole output to the sink at their end)
  if (out_spp) {
    if ((rc = sc->stage_spp.reserve((size_t)npix * sizeof(int32_t)))) return rc;
    HIPC(hipMemcpyAsync(sc->stage_spp.p, sc->out_spp.p, (size_t)npix * sizeof(int32_t), hipMemcpyDeviceToHost,
                        sc->stream));
  }
  HIPC(hipStreamSynchronize(sc->stream));
  int64_t r = 0;  // packed row
  for (int64_t b = stripe; b < nblk; b += N) {
    const int64_t y0 = b * R, rows = std::min<int64_t>(R, H - y0);
    if (!direct)
      std::memcpy(out_rgb + (size_t)y0 * W * 3, (const char*)sc->stage_rgb.p + (size_t)r * row_rgb,
                  (size_t)rows * row_rgb);
    if (out_spp)
      std::memcpy(out_spp + (size_t)y0 * W, (const char*)sc->stage_spp.p + (size_t)r * row_spp,
                  (size_t)rows * row_spp);
    r += rows;
  }
  if (g_debug_host) {
    static thread_local double t_prev_out = 0;  // (rtx_render_multi: one thread per device)
    const double t_out = host_us();
    fprintf(stderr,
            "rtx host: device %d: since last frame %.1f us | to first launch %.1f | launches %.1f | sync wait %.1f | "
            "after %.1f\n",
            sc->device, t_prev_out > 0 ? t_in - t_prev_out : -1.0, g_t_launch - t_in, g_t_sync0 - g_t_launch,
            g_t_sync1 - g_t_sync0, t_out - g_t_sync1);
    t_prev_out = t_out;
  }
  return RTX_OK;
}
}  // namespace

int rtx_render_multi(rtx_scene* const* scenes, int32_t n, const rtx_camera* cam, const rtx_render_params* prm,
                     double* out_rgb, int32_t* out_spp, rtx_stats* stats, rtx_stats* per_scene) {
  if (!scenes || n <= 0 || !cam || !prm || !out_rgb) return fail(RTX_ERR_INVALID, "bad argument");
  for (int32_t k = 0; k < n; k++)
    if (!scenes[k]) return fail(RTX_ERR_INVALID, "scene is NULL");
  for (int32_t j = 0; j < n; j++)
    for (int32_t k = j + 1; k < n; k++)
      if (scenes[j] == scenes[k]) return fail(RTX_ERR_INVALID, "a scene appears twice (one scene per render thread)");
  rtx_render_params base = *prm;
  if (base.stripe_rows <= 0) base.stripe_rows = 8;
  if (base.stripe_count <= 0) base.stripe_count = n, base.stripe_index = 0;
  if (base.stripe_index < 0 || base.stripe_index + n > base.stripe_count)
    return fail(RTX_ERR_INVALID, "stripes stripe_index .. stripe_index + n - 1 must lie below stripe_count");
  std::vector<int> rc(n, RTX_OK);
  std::vector<std::string> msg(n);
  std::vector<rtx_stats> st(n);
  auto work = [&](int k) {
    st[k] = rtx_stats{};
    rc[k] = render_stripes_to_host(scenes[k], cam, &base, base.stripe_index + k, out_rgb, out_spp, &st[k]);
    if (rc[k] != RTX_OK) msg[k] = g_err;  // rtx_last_error is per thread
  };
  if (n == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    th.reserve(n);
    for (int k = 0; k < n; k++) th.emplace_back(work, k);
    for (auto& t : th) t.join();
  }
  for (int k = 0; k < n; k++)
    if (rc[k] != RTX_OK) return fail(rc[k], "device " + std::to_string(scenes[k]->device) + ": " + msg[k]);
  if (per_scene)
    for (int k = 0; k < n; k++) per_scene[k] = st[k];
  if (stats) {
    rtx_stats a{};
    for (int k = 0; k < n; k++) {
      a.rays_primary += st[k].rays_primary, a.rays_total += st[k].rays_total, a.paths += st[k].paths;
      a.kernel_ms = std::max(a.kernel_ms, st[k].kernel_ms);
      a.hot_kernel_ms = std::max(a.hot_kernel_ms, st[k].hot_kernel_ms);
      a.hot_launches += st[k].hot_launches, a.node_visits += st[k].node_visits, a.prim_tests += st[k].prim_tests;
      a.wave_node_iters += st[k].wave_node_iters, a.wave_prim_iters += st[k].wave_prim_iters;
      a.tri_tests += st[k].tri_tests, a.sphere_tests += st[k].sphere_tests;
      a.rays_recorded += st[k].rays_recorded;
      a.wave_rounds += st[k].wave_rounds, a.wave_rounds_idle += st[k].wave_rounds_idle;
      a.wave_lanes_live += st[k].wave_lanes_live;
      a.node_bytes = st[k].node_bytes, a.parked |= st[k].parked, a.build |= st[k].build;
    }
    *stats = a;
  }
  return RTX_OK;
}

// ---- P3 output on the device (wavefront.cc:238-241, core/color.h:18-33) ----
static std::string p3_header(int64_t w, int64_t h) {
  return "P3\n" + std::to_string(w) + " " + std::to_string(h) + "\n255\n";
}

size_t rtx_p3_max_bytes(int32_t w, int32_t h) {
  if (w <= 0 || h <= 0) return 0;
  return p3_header(w, h).size() + (size_t)w * (size_t)h * rtxp3::kMaxLine;
}

// body of d_rgb into sc->p3_body; *len = body bytes
static int p3_encode(rtx_scene* sc, const double* d_rgb, int64_t npix, size_t* len, hipStream_t s) {
  if ((uint64_t)npix * rtxp3::kMaxLine > 0xFFFFFFFFull) return fail(RTX_ERR_INVALID, "P3 output above 4 GiB");
  int rc;
  if ((rc = sc->p3_scratch.reserve(rtxp3::scratch_bytes(std::max<int64_t>(1, npix))))) return rc;
  if ((rc = sc->p3_body.reserve(std::max<int64_t>(1, npix) * rtxp3::kMaxLine))) return rc;
  HIPC(rtxp3::encode_body(d_rgb, npix, sc->p3_scratch.p, (char*)sc->p3_body.p, len, s));
  return RTX_OK;
}

int rtx_encode_p3_device(rtx_scene* sc, const double* d_rgb, int32_t w, int32_t h, char* d_out, size_t cap,
                         size_t* out_len, void* stream) {
  if (!sc || !d_rgb || !d_out || !out_len || w <= 0 || h <= 0) return fail(RTX_ERR_INVALID, "bad argument");
  if (cap < rtx_p3_max_bytes(w, h)) return fail(RTX_ERR_INVALID, "output buffer below rtx_p3_max_bytes");
  HIPC(hipSetDevice(sc->device));
  hipStream_t s = stream ? (hipStream_t)stream : sc->stream;
  const std::string hd = p3_header(w, h);
  size_t body = 0;
  int rc;
  if ((rc = p3_encode(sc, d_rgb, (int64_t)w * h, &body, s))) return rc;
  HIPC(hipMemcpyAsync(d_out, hd.data(), hd.size(), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_out + hd.size(), sc->p3_body.p, body, hipMemcpyDeviceToDevice, s));
  HIPC(hipStreamSynchronize(s));
  *out_len = hd.size() + body;
  return RTX_OK;
}

int rtx_encode_p3(rtx_scene* sc, const double* rgb, int32_t w, int32_t h, char* out, size_t cap, size_t* out_len) {
  if (!sc || !rgb || !out || !out_len || w <= 0 || h <= 0) return fail(RTX_ERR_INVALID, "bad argument");
  if (cap < rtx_p3_max_bytes(w, h)) return fail(RTX_ERR_INVALID, "output buffer below rtx_p3_max_bytes");
  HIPC(hipSetDevice(sc->device));
  const int64_t npix = (int64_t)w * h;
  int rc;
  if ((rc = sc->out_rgb.reserve(npix * 3 * sizeof(double)))) return rc;
  HIPC(hipMemcpyAsync(sc->out_rgb.p, rgb, npix * 3 * sizeof(double), hipMemcpyHostToDevice, sc->stream));
  const std::string hd = p3_header(w, h);
  size_t body = 0;
  if ((rc = p3_encode(sc, sc->out_rgb.as<double>(), npix, &body, sc->stream))) return rc;
  std::memcpy(out, hd.data(), hd.size());
  HIPC(hipMemcpyAsync(out + hd.size(), sc->p3_body.p, body, hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  *out_len = hd.size() + body;
  return RTX_OK;
}

int rtx_render_p3(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, char* out, size_t cap,
                  size_t* out_len, double* rgb, int32_t* spp, rtx_stats* stats) {
  if (!sc || !cam || !prm || !out || !out_len) return fail(RTX_ERR_INVALID, "NULL argument");
  PixelMap map;
  std::string err;
  const int64_t npix = subset_pixels(cam, prm, map, err);
  if (npix < 0) return fail(RTX_ERR_INVALID, err);
  const std::string hd = p3_header(map.w, map.h);
  if (cap < hd.size() + (size_t)npix * rtxp3::kMaxLine) return fail(RTX_ERR_INVALID, "output buffer below rtx_p3_max_bytes");
  HIPC(hipSetDevice(sc->device));
  int rc;
  if ((rc = sc->out_rgb.reserve(std::max<int64_t>(1, npix) * 3 * sizeof(double)))) return rc;
  if ((rc = sc->out_spp.reserve(std::max<int64_t>(1, npix) * sizeof(int32_t)))) return rc;
  if ((rc = rtx_render_device(sc, cam, prm, sc->out_rgb.as<double>(), sc->out_spp.as<int32_t>(), stats, sc->stream)))
    return rc;
  size_t body = 0;
  if ((rc = p3_encode(sc, sc->out_rgb.as<double>(), npix, &body, sc->stream))) return rc;
  std::memcpy(out, hd.data(), hd.size());
  HIPC(hipMemcpyAsync(out + hd.size(), sc->p3_body.p, body, hipMemcpyDeviceToHost, sc->stream));
  if (rgb) HIPC(hipMemcpyAsync(rgb, sc->out_rgb.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
  if (spp) HIPC(hipMemcpyAsync(spp, sc->out_spp.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  *out_len = hd.size() + body;
  return RTX_OK;
}

// ---- films: a frame rendered in steps, resolved on demand, saved and continued ----------------
// (DESIGN.md "Film")
namespace {
// A film's calls need its scene alive, on the film's device.
int film_live(const rtx_film* f) {
  if (!f) return fail(RTX_ERR_INVALID, "film is NULL");
  if (!f->sc) return fail(RTX_ERR_INVALID, "the film's scene was destroyed");
  if (f->sc->device != f->device) return fail(RTX_ERR_INVALID, "the film's scene is on another device");
  if (f->sc->epoch != f->epoch) return fail(RTX_ERR_INVALID, "scene changed since the film was created");
  return RTX_OK;
}
// the blob's sampler field: 0 wavefront family, 1 megakernel, 2 / 3 a sampled film's NEE / MIS
int film_sampler(const rtx_film* f) {
  if (f->estimator) return f->estimator == RTX_ESTIMATOR_MIS ? 3 : 2;
  return f->prm.mode == RTX_MODE_MEGAKERNEL ? 1 : 0;
}
FilmHeader film_header(const rtx_film* f) {
  FilmHeader h{};
  std::memcpy(h.magic, kFilmMagic, sizeof h.magic);
  h.version = kFilmVersion, h.header_bytes = kFilmHeaderBytes;
  const PixelMap& m = f->map;
  h.W = m.W, h.H = m.H, h.stripes = m.stripes, h.x0 = m.x0, h.y0 = m.y0, h.w = m.w, h.h = m.h;
  if (m.stripes) h.srows = m.srows, h.sidx = m.sidx, h.scount = m.scount;
  h.seed = f->prm.seed, h.max_depth = f->prm.max_depth, h.adaptive = f->prm.adaptive ? 1 : 0;
  h.min_spp = f->prm.min_spp, h.sampler = film_sampler(f), h.rel_threshold = f->prm.rel_threshold;
  h.done = f->done, h.npix = f->npix;
  return h;
}
int film_pack(const rtx_film* f, int to_body, hipStream_t s) {
  const int64_t n = 3 * f->npix;
  if (n == 0) return RTX_OK;
  const int adaptive = f->prm.adaptive ? 1 : 0;
  hipLaunchKernelGGL(k_film_pack, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, f->px(),
                     film_body_at(f->stage.p, f->npix, adaptive), f->npix, adaptive, to_body);
  HIPC(hipGetLastError());
  return RTX_OK;
}
int film_resolve_on(const rtx_film* f, double* d_rgb, int32_t* d_spp, hipStream_t s) {
  if (f->npix == 0) return RTX_OK;
  hipLaunchKernelGGL(k_film_resolve, dim3((unsigned)((f->npix + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, f->px(),
                     f->npix, film_sampler(f), f->done, d_rgb, d_spp);
  HIPC(hipGetLastError());
  return RTX_OK;
}
// The film of checked parameters: the pixel subset, the zeroed state, the scene's record of it.
// estimator: 0, or a sampled film's (rtx_film_create_sampled).
int film_make(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, int32_t estimator, rtx_film** out) {
  auto f = std::make_unique<rtx_film>();
  f->estimator = estimator;
  std::string err;
  f->npix = subset_pixels(cam, prm, f->map, err);
  if (f->npix < 0) return fail(RTX_ERR_INVALID, err);
  f->sc = sc, f->device = sc->device, f->cam = *cam, f->prm = *prm;
  f->epoch = sc->epoch;
  f->prm.spp = 0;
  f->prm.adaptive = prm->adaptive ? 1 : 0;
  HIPC(hipSetDevice(sc->device));
  const size_t n = (size_t)std::max<int64_t>(1, f->npix);
  int rc = RTX_OK;
  struct Plan {
    DevBuf* b;
    size_t bytes;
  } plan[] = {{&f->sum, n * 3 * sizeof(double)},
              {&f->mean, f->prm.adaptive ? n * 3 * sizeof(double) : 0},
              {&f->m2, f->prm.adaptive ? n * 3 * sizeof(double) : 0},
              {&f->samples, n * sizeof(int32_t)},
              {&f->conv, n}};
  for (const Plan& q : plan) {
    if (!q.bytes) continue;
    if ((rc = q.b->reserve(q.bytes))) break;
    if (hipMemsetAsync(q.b->p, 0, q.bytes, sc->stream) != hipSuccess) {
      rc = fail(RTX_ERR_HIP, "hipMemsetAsync of the film's state failed");
      break;
    }
  }
  if (rc) return rc;
  sc->films.push_back(f.get());
  *out = f.release();
  return RTX_OK;
}
}  // namespace

int rtx_film_create(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, rtx_film** out) {
  if (!sc || !cam || !prm || !out) return fail(RTX_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (prm->max_depth < 0) return fail(RTX_ERR_INVALID, "negative max_depth");
  if (prm->mode < RTX_MODE_WAVEFRONT || prm->mode > RTX_MODE_MEGAKERNEL) return fail(RTX_ERR_INVALID, "bad mode");
  // AdaptiveSampler's budget is spp + 1 samples of every unfinished pixel, decided inside one
  // call: a prefix of it is not a smaller render
  if (prm->adaptive && prm->mode == RTX_MODE_MEGAKERNEL)
    return fail(RTX_ERR_INVALID, "megakernel films are fixed-spp only (AdaptiveSampler does not compose across calls)");
  return film_make(sc, cam, prm, 0, out);
}

int rtx_film_create_sampled(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, int32_t estimator,
                            rtx_film** out) {
  if (!sc || !cam || !prm || !out) return fail(RTX_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (estimator != RTX_ESTIMATOR_NEE && estimator != RTX_ESTIMATOR_MIS) return fail(RTX_ERR_INVALID, "bad estimator");
  if (prm->max_depth < 0) return fail(RTX_ERR_INVALID, "negative max_depth");
  int rc;
  if ((rc = nee_depth_check(prm->max_depth, estimator == RTX_ESTIMATOR_MIS))) return rc;
  if (prm->precision != RTX_PREC_PARITY && prm->precision != RTX_PREC_FAST)
    return fail(RTX_ERR_INVALID, "sampled film: bad precision");
  // spp, mode, flags and samples_per_group are not read: the film keeps the values a plain
  // wavefront film has, so the two describe themselves alike
  rtx_render_params q = *prm;
  q.mode = RTX_MODE_WAVEFRONT, q.flags = 0, q.samples_per_group = 0;
  return film_make(sc, cam, &q, estimator, out);
}

int rtx_film_destroy(rtx_film* f) {
  if (!f) return RTX_OK;
  if (f->sc) {
    (void)hipSetDevice(f->device);
    (void)hipStreamSynchronize(f->sc->stream);  // a render queued without stats may still write the state
    auto& v = f->sc->films;
    v.erase(std::remove(v.begin(), v.end(), f), v.end());
  }
  delete f;  // (its buffers, if it still has any, go with it)
  return RTX_OK;
}

int rtx_film_samples(const rtx_film* f, int32_t* done) {
  if (!f || !done) return fail(RTX_ERR_INVALID, "NULL argument");
  *done = f->done;
  return RTX_OK;
}

int rtx_film_reset(rtx_film* f) {
  if (!f) return fail(RTX_ERR_INVALID, "film is NULL");
  if (!f->sc) return fail(RTX_ERR_INVALID, "the film's scene was destroyed");
  if (f->sc->device != f->device) return fail(RTX_ERR_INVALID, "the film's scene is on another device");
  HIPC(hipSetDevice(f->device));
  for (DevBuf* b : {&f->sum, &f->mean, &f->m2, &f->samples, &f->conv})
    if (b->p) HIPC(hipMemsetAsync(b->p, 0, b->n, f->sc->stream));
  f->done = 0;
  f->active = -1;
  f->aov_ready = false;
  f->epoch = f->sc->epoch;
  return RTX_OK;
}

int rtx_film_render(rtx_film* f, int32_t budget, rtx_stats* stats) {
  int rc;
  if ((rc = film_live(f))) return rc;
  if (budget < 0) return fail(RTX_ERR_INVALID, "negative budget");
  if (stats) *stats = rtx_stats{};
  if (budget <= f->done) return RTX_OK;
  if (f->estimator) {  // a sampled film: its own groups (rtx_film_sampled.h)
    if ((rc = film_sampled_render(f, budget, stats))) return rc;
    f->done = budget;
    return RTX_OK;
  }
  rtx_render_params q = f->prm;
  q.spp = budget;
  const FilmRun run{f->px(), f->done};
  if ((rc = render_device_impl(f->sc, &f->cam, &q, nullptr, nullptr, stats, f->sc->stream, nullptr, &run))) return rc;
  f->done = budget;
  return RTX_OK;
}

int rtx_film_resolve_device(rtx_film* f, double* d_rgb, int32_t* d_spp, void* stream) {
  int rc;
  if ((rc = film_live(f))) return rc;
  if (!d_rgb) return fail(RTX_ERR_INVALID, "NULL argument");
  HIPC(hipSetDevice(f->device));
  hipStream_t s = stream ? (hipStream_t)stream : f->sc->stream;
  if (s != f->sc->stream) HIPC(hipStreamSynchronize(f->sc->stream));  // the film's renders run on the scene's stream
  return film_resolve_on(f, d_rgb, d_spp, s);
}

int rtx_film_resolve(rtx_film* f, double* rgb, int32_t* spp) {
  int rc;
  if ((rc = film_live(f))) return rc;
  if (!rgb) return fail(RTX_ERR_INVALID, "NULL argument");
  rtx_scene* sc = f->sc;
  HIPC(hipSetDevice(f->device));
  const int64_t npix = f->npix;
  if ((rc = sc->out_rgb.reserve(std::max<int64_t>(1, npix) * 3 * sizeof(double)))) return rc;
  if ((rc = sc->out_spp.reserve(std::max<int64_t>(1, npix) * sizeof(int32_t)))) return rc;
  if ((rc = film_resolve_on(f, sc->out_rgb.as<double>(), sc->out_spp.as<int32_t>(), sc->stream))) return rc;
  HIPC(hipMemcpyAsync(rgb, sc->out_rgb.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
  if (spp) HIPC(hipMemcpyAsync(spp, sc->out_spp.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

int rtx_film_p3(rtx_film* f, char* out, size_t cap, size_t* out_len) {
  int rc;
  if ((rc = film_live(f))) return rc;
  if (!out || !out_len) return fail(RTX_ERR_INVALID, "NULL argument");
  rtx_scene* sc = f->sc;
  const int64_t npix = f->npix;
  const std::string hd = p3_header(f->map.w, f->map.h);
  if (cap < hd.size() + (size_t)npix * rtxp3::kMaxLine) return fail(RTX_ERR_INVALID, "output buffer below rtx_p3_max_bytes");
  HIPC(hipSetDevice(f->device));
  if ((rc = sc->out_rgb.reserve(std::max<int64_t>(1, npix) * 3 * sizeof(double)))) return rc;
  if ((rc = film_resolve_on(f, sc->out_rgb.as<double>(), nullptr, sc->stream))) return rc;
  size_t body = 0;
  if ((rc = p3_encode(sc, sc->out_rgb.as<double>(), npix, &body, sc->stream))) return rc;
  std::memcpy(out, hd.data(), hd.size());
  HIPC(hipMemcpyAsync(out + hd.size(), sc->p3_body.p, body, hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  *out_len = hd.size() + body;
  return RTX_OK;
}

size_t rtx_film_state_bytes(const rtx_film* f) {
  if (!f) {
    (void)fail(RTX_ERR_INVALID, "film is NULL");
    return 0;
  }
  return kFilmHeaderBytes + film_body_bytes(f->npix, f->prm.adaptive);
}

int rtx_film_save(const rtx_film* f, void* blob, size_t cap, size_t* len) {
  int rc;
  if ((rc = film_live(f))) return rc;
  if (!blob || !len) return fail(RTX_ERR_INVALID, "NULL argument");
  const size_t body = film_body_bytes(f->npix, f->prm.adaptive);
  if (cap < kFilmHeaderBytes + body) return fail(RTX_ERR_INVALID, "blob buffer below rtx_film_state_bytes");
  HIPC(hipSetDevice(f->device));
  hipStream_t s = f->sc->stream;
  if ((rc = f->stage.reserve(std::max<size_t>(16, body)))) return rc;
  if ((rc = film_pack(f, 1, s))) return rc;
  if (body) HIPC(hipMemcpyAsync((char*)blob + kFilmHeaderBytes, f->stage.p, body, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  const FilmHeader h = film_header(f);
  std::memcpy(blob, &h, sizeof h);
  *len = kFilmHeaderBytes + body;
  return RTX_OK;
}

int rtx_film_blob_check(const void* blob, size_t len) {
  const std::string e = film_blob_error(blob, len);
  return e.empty() ? RTX_OK : fail(RTX_ERR_INVALID, "film blob: " + e);
}

int rtx_film_load(rtx_film* f, const void* blob, size_t len) {
  int rc;
  if ((rc = film_live(f))) return rc;
  FilmHeader b;
  const std::string e = film_blob_error(blob, len, &b);
  if (!e.empty()) return fail(RTX_ERR_INVALID, "film blob: " + e);
  // everything that decides a sample's value or a pixel's place must be the film's own
  const FilmHeader h = film_header(f);
  const char* field = nullptr;
  if (b.W != h.W || b.H != h.H) field = "image size";
  else if (b.stripes != h.stripes || b.x0 != h.x0 || b.y0 != h.y0 || b.w != h.w || b.h != h.h || b.srows != h.srows ||
           b.sidx != h.sidx || b.scount != h.scount || b.npix != h.npix)
    field = "pixel map";
  else if (b.seed != h.seed) field = "seed";
  else if (b.max_depth != h.max_depth) field = "max_depth";
  else if (b.adaptive != h.adaptive) field = "adaptive";
  else if (b.sampler != h.sampler) field = "sampler (wavefront family / megakernel)";
  else if (h.adaptive && b.min_spp != h.min_spp) field = "min_spp";
  else if (h.adaptive && std::memcmp(&b.rel_threshold, &h.rel_threshold, sizeof(double)) != 0) field = "rel_threshold";
  if (field) return fail(RTX_ERR_INVALID, std::string("film blob: ") + field + " differs from the film's");
  const size_t body = film_body_bytes(f->npix, h.adaptive);
  HIPC(hipSetDevice(f->device));
  hipStream_t s = f->sc->stream;
  if ((rc = f->stage.reserve(std::max<size_t>(16, body)))) return rc;
  if (body) HIPC(hipMemcpyAsync(f->stage.p, (const char*)blob + kFilmHeaderBytes, body, hipMemcpyHostToDevice, s));
  if ((rc = film_pack(f, 0, s))) return rc;
  HIPC(hipStreamSynchronize(s));  // the blob is the caller's memory
  f->done = b.done;
  f->active = -1;
  return RTX_OK;
}

// ---- first-hit AOVs and the denoiser (rtx_denoise.h, DESIGN.md "AOVs and the denoiser") -------
namespace {
const rtx_denoise_params kDenoiseDefaults{5, RTX_DENOISE_DEMODULATE, 64.0, 0.05, 4.0};
// Validated parameters as the kernels take them; *npix = w * h.
int denoise_check(int32_t w, int32_t h, const rtx_denoise_params* p, rtxdn::FilterParams& f, int64_t* npix) {
  if (w <= 0 || h <= 0) return fail(RTX_ERR_INVALID, "denoise: image size <= 0");
  if ((int64_t)w * h >= 0x80000000ll) return fail(RTX_ERR_INVALID, "denoise: image of 2^31 pixels or more");
  const rtx_denoise_params& q = p ? *p : kDenoiseDefaults;
  if (q.iterations < 0 || q.iterations > rtxdn::kMaxIterations) return fail(RTX_ERR_INVALID, "denoise: iterations outside 0..8");
  if (q.flags & ~RTX_DENOISE_DEMODULATE) return fail(RTX_ERR_INVALID, "denoise: unknown flags");
  if (!(q.normal_power > 0) || !(q.sigma_depth > 0) || !(q.sigma_color > 0) || !std::isfinite(q.normal_power) ||
      !std::isfinite(q.sigma_depth) || !std::isfinite(q.sigma_color))
    return fail(RTX_ERR_INVALID, "denoise: normal_power and the sigmas must be positive");
  f = rtxdn::FilterParams{q.iterations, q.flags, (float)q.normal_power, (float)q.sigma_depth, (float)q.sigma_color};
  *npix = (int64_t)w * h;
  return RTX_OK;
}
int denoise_work(rtx_scene* sc, int64_t npix, bool guides) {
  int rc;
  for (DevBuf& b : sc->dn_work)
    if ((rc = b.reserve((size_t)npix * sizeof(float4)))) return rc;
  if (guides)
    for (DevBuf* b : {&sc->dn_guide, &sc->dn_alb})
      if ((rc = b->reserve((size_t)npix * sizeof(float4)))) return rc;
  return RTX_OK;
}
}  // namespace

int rtx_denoise_params_default(rtx_denoise_params* out) {
  if (!out) return fail(RTX_ERR_INVALID, "NULL argument");
  *out = kDenoiseDefaults;
  return RTX_OK;
}

int rtx_denoise_device(rtx_scene* sc, int32_t w, int32_t h, const double* d_rgb, const double* d_albedo,
                       const double* d_normal, const double* d_depth, const double* d_variance,
                       const rtx_denoise_params* p, double* d_out, void* stream) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!d_rgb || !d_albedo || !d_normal || !d_depth || !d_out) return fail(RTX_ERR_INVALID, "NULL buffer");
  rtxdn::FilterParams f;
  int64_t npix;
  int rc;
  if ((rc = denoise_check(w, h, p, f, &npix))) return rc;
  HIPC(hipSetDevice(sc->device));
  hipStream_t s = stream ? (hipStream_t)stream : sc->stream;
  if (s != sc->stream) HIPC(hipStreamSynchronize(sc->stream));  // the working buffers may still be in use there
  if (f.iterations > 0) {
    if ((rc = denoise_work(sc, npix, true))) return rc;
    HIPC(rtxdn::pack_guides(d_normal, d_depth, d_albedo, npix, sc->dn_guide.as<float4>(), sc->dn_alb.as<float4>(), s));
  }
  HIPC(rtxdn::filter(w, h, d_rgb, d_variance, sc->dn_guide.as<float4>(), sc->dn_alb.as<float4>(),
                     sc->dn_work[0].as<float4>(), sc->dn_work[1].as<float4>(), f, d_out, s));
  return RTX_OK;
}

int rtx_denoise(rtx_scene* sc, int32_t w, int32_t h, const double* rgb, const double* albedo, const double* normal,
                const double* depth, const double* variance, const rtx_denoise_params* p, double* out) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!rgb || !albedo || !normal || !depth || !out) return fail(RTX_ERR_INVALID, "NULL buffer");
  rtxdn::FilterParams f;
  int64_t npix;
  int rc;
  if ((rc = denoise_check(w, h, p, f, &npix))) return rc;
  HIPC(hipSetDevice(sc->device));
  if ((rc = sc->dn_in.reserve((size_t)npix * 11 * sizeof(double)))) return rc;
  double* d = sc->dn_in.as<double>();  // rgb 3 n, albedo 3 n, normal 3 n, depth n, variance n
  double *d_alb = d + 3 * npix, *d_nrm = d + 6 * npix, *d_dep = d + 9 * npix, *d_var = d + 10 * npix;
  hipStream_t s = sc->stream;
  const size_t one = (size_t)npix * sizeof(double);
  HIPC(hipMemcpyAsync(d, rgb, 3 * one, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_alb, albedo, 3 * one, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_nrm, normal, 3 * one, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_dep, depth, one, hipMemcpyHostToDevice, s));
  if (variance) HIPC(hipMemcpyAsync(d_var, variance, one, hipMemcpyHostToDevice, s));
  if ((rc = rtx_denoise_device(sc, w, h, d, d_alb, d_nrm, d_dep, variance ? d_var : nullptr, p, d, s))) return rc;
  HIPC(hipMemcpyAsync(out, d, 3 * one, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return RTX_OK;
}

namespace {
// The film's denoised frame into sc->out_rgb (device), enqueued on the scene's stream.
int film_denoise_on(rtx_film* f, const rtx_denoise_params* p) {
  int rc;
  if ((rc = film_live(f))) return rc;
  if (f->map.stripes) return fail(RTX_ERR_INVALID, "a stripe film cannot be denoised: stripes are not adjacent rows");
  rtx_scene* sc = f->sc;
  const int64_t npix = f->npix;
  if ((rc = sc->out_rgb.reserve(std::max<int64_t>(1, npix) * 3 * sizeof(double)))) return rc;
  if (npix == 0) return RTX_OK;
  rtxdn::FilterParams fp;
  int64_t n;
  if ((rc = denoise_check(f->map.w, f->map.h, p, fp, &n))) return rc;
  HIPC(hipSetDevice(f->device));
  hipStream_t s = sc->stream;
  if ((rc = film_resolve_on(f, sc->out_rgb.as<double>(), nullptr, s))) return rc;
  if (fp.iterations == 0) return RTX_OK;  // the resolved frame itself
  if ((rc = denoise_work(sc, npix, false))) return rc;
  if (!f->aov_ready) {
    for (DevBuf* b : {&f->dn_guide, &f->dn_alb})
      if ((rc = b->reserve((size_t)npix * sizeof(float4)))) return rc;
    if ((rc = sc->aov_f64.reserve((size_t)npix * 7 * sizeof(double)))) return rc;
    double* a = sc->aov_f64.as<double>();
    if ((rc = aov_on(sc, &f->cam, f->map, npix, f->prm.precision, a, a + 3 * npix, a + 6 * npix, s))) return rc;
    HIPC(rtxdn::pack_guides(a + 3 * npix, a + 6 * npix, a, npix, f->dn_guide.as<float4>(), f->dn_alb.as<float4>(), s));
    f->aov_ready = true;
  }
  const double* d_var = nullptr;
  if (f->prm.adaptive) {  // a fixed-spp film keeps no M2
    if ((rc = sc->dn_var.reserve((size_t)npix * sizeof(double)))) return rc;
    hipLaunchKernelGGL(k_film_variance, dim3((unsigned)((npix + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, f->px(), npix,
                       (const float4*)f->dn_alb.as<float4>(), fp.flags & RTX_DENOISE_DEMODULATE, sc->dn_var.as<double>());
    HIPC(hipGetLastError());
    d_var = sc->dn_var.as<double>();
  }
  HIPC(rtxdn::filter(f->map.w, f->map.h, sc->out_rgb.as<double>(), d_var, f->dn_guide.as<float4>(),
                     f->dn_alb.as<float4>(), sc->dn_work[0].as<float4>(), sc->dn_work[1].as<float4>(), fp,
                     sc->out_rgb.as<double>(), s));
  return RTX_OK;
}
}  // namespace

int rtx_film_denoise(rtx_film* f, const rtx_denoise_params* p, double* out_rgb) {
  int rc;
  if ((rc = film_live(f))) return rc;
  if (!out_rgb) return fail(RTX_ERR_INVALID, "NULL argument");
  if ((rc = film_denoise_on(f, p))) return rc;
  rtx_scene* sc = f->sc;
  HIPC(hipMemcpyAsync(out_rgb, sc->out_rgb.p, (size_t)f->npix * 3 * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

int rtx_film_denoise_p3(rtx_film* f, const rtx_denoise_params* p, char* out, size_t cap, size_t* out_len) {
  int rc;
  if ((rc = film_live(f))) return rc;
  if (!out || !out_len) return fail(RTX_ERR_INVALID, "NULL argument");
  rtx_scene* sc = f->sc;
  const std::string hd = p3_header(f->map.w, f->map.h);
  if (cap < hd.size() + (size_t)f->npix * rtxp3::kMaxLine) return fail(RTX_ERR_INVALID, "output buffer below rtx_p3_max_bytes");
  if ((rc = film_denoise_on(f, p))) return rc;
  size_t body = 0;
  if ((rc = p3_encode(sc, sc->out_rgb.as<double>(), f->npix, &body, sc->stream))) return rc;
  std::memcpy(out, hd.data(), hd.size());
  HIPC(hipMemcpyAsync(out + hd.size(), sc->p3_body.p, body, hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  *out_len = hd.size() + body;
  return RTX_OK;
}

// write_color (core/color.h:10-33): sqrt gamma, clamp [0, 0.999], int(256 x).
int rtx_write_ppm(const char* path, const double* rgb, int32_t w, int32_t h) {
  if (!path || !rgb || w <= 0 || h <= 0) return fail(RTX_ERR_INVALID, "bad argument");
  FILE* f = std::fopen(path, "w");
  if (!f) return fail(RTX_ERR_IO, std::string("cannot write ") + path);
  std::fprintf(f, "P3\n%d %d\n255\n", w, h);
  for (int64_t i = 0; i < (int64_t)w * h; i++) {
    int b[3];
    for (int c = 0; c < 3; c++) {
      double x = rgb[3 * i + c];
      x = x > 0 ? std::sqrt(x) : 0;
      x = x < 0.0 ? 0.0 : (x > 0.999 ? 0.999 : x);
      b[c] = int(256 * x);
    }
    std::fprintf(f, "%d %d %d\n", b[0], b[1], b[2]);
  }
  std::fclose(f);
  return RTX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// Self-check of the restated small-argument cos/sin (rtxd::sincos_small, used by the plain
// kernel's Lambertian sampling) against the device library's cos() and sin(): n arguments
// phi = 2*pi*u with u the reference's 53-bit uniform draws (a 64-bit mix of seed and index,
// top 53 bits), plus the ends of [0, 1) and the quadrant boundaries.  Test hook only (not in
// rtx.h): tests/test_gpu_timed.py.
namespace {
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__global__ void k_check_sincos(int64_t n, uint64_t seed, unsigned long long* bad, double* first_bad) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + 64; i += (int64_t)gridDim.x * blockDim.x) {
    double u;
    if (i < n) {
      u = (double)(mix64(seed + (uint64_t)i) >> 11) * 0x1.0p-53;
    } else {  // 0, the largest draw, and 1/4, 1/2, 3/4 (and their neighbours)
      const int j = (int)(i - n);
      const double base[5] = {0.0, 1.0, 0.25, 0.5, 0.75};
      u = base[j % 5];
      const int steps = j / 5 - 6;  // -6 .. +6 draws around the point
      u += steps * 0x1.0p-53;
      if (u < 0.0 || u >= 1.0) continue;
    }
    const double phi = 2.0 * rtxd::kPi * u;
    double s, c;
    rtxd::sincos_small(phi, s, c);
    const double c0 = cos(phi), s0 = sin(phi);
    if (__double_as_longlong(c) != __double_as_longlong(c0) || __double_as_longlong(s) != __double_as_longlong(s0)) {
      if (atomicAdd(bad, 1ull) == 0) *first_bad = u;
    }
  }
}
}  // namespace

extern "C" int rtx_internal_check_sincos(int device, int64_t n, uint64_t seed, int64_t* mismatches,
                                         double* first_bad) {
  if (n < 0 || !mismatches) return fail(RTX_ERR_INVALID, "bad argument");
  HIPC(hipSetDevice(device));
  DevBuf b;
  int rc;
  if ((rc = b.reserve(2 * sizeof(unsigned long long)))) return rc;
  HIPC(hipMemset(b.p, 0, 2 * sizeof(unsigned long long)));
  unsigned long long* bad = b.as<unsigned long long>();
  hipLaunchKernelGGL(k_check_sincos, dim3(1024), dim3(256), 0, nullptr, n, seed, bad, (double*)(bad + 1));
  HIPC(hipGetLastError());
  unsigned long long h[2];
  HIPC(hipMemcpy(h, bad, sizeof(h), hipMemcpyDeviceToHost));
  *mismatches = (int64_t)h[0];
  if (first_bad) std::memcpy(first_bad, &h[1], sizeof(double));
  return RTX_OK;
}

// Test / tuning hook (not in rtx.h): overrides of the adaptive phases' constants for the
// renders that follow in this process (0 / negative restores a default): the smallest phase,
// the largest batch of a pixel, the first pass's kernel (1 the phase kernel, 0 the uniform-group
// one) and the batch margin's growth per phase.  Results never depend on them, only the amount
// of work and the number of phases do (tests/test_gpu_timed.py runs the full budgets through
// forced small workspaces).
extern "C" int rtx_internal_adapt_tune(int64_t phase_slots, int32_t phase_kcap, int32_t first_map, double phase_mstep,
                                       double margin1, double pool_w) {
  if (phase_slots < 0 || phase_kcap < 0 || first_map > 1) return fail(RTX_ERR_INVALID, "bad tuning value");
  g_tune = AdaptTune{phase_slots, phase_kcap, first_map, phase_mstep, margin1, pool_w};
  return RTX_OK;
}

namespace {
// the pixel statistics (channel-major on the device) to the caller's [npix][3] / [npix] arrays
int read_pixels(const PixelSoA& px, int64_t npix, double* sum, double* mean, double* m2, int32_t* samples,
                uint8_t* conv) {
  std::vector<double> h(3 * (size_t)npix);
  const double* src[3] = {px.sum, px.mean, px.m2};
  double* dst[3] = {sum, mean, m2};
  for (int a = 0; a < 3; a++) {
    if (!dst[a]) continue;
    HIPC(hipMemcpy(h.data(), src[a], h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < npix; p++)
      for (int c = 0; c < 3; c++) dst[a][3 * p + c] = h[(size_t)c * npix + p];
  }
  if (samples) HIPC(hipMemcpy(samples, px.samples, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (conv) HIPC(hipMemcpy(conv, px.conv, npix, hipMemcpyDeviceToHost));
  return RTX_OK;
}
}  // namespace

// Test hook (not in rtx.h): render_adaptive's own phase loop (record, plan, floor, scan, expand,
// the host's read of the slot and pixel counts, the workspace sizing; rtx_internal_adapt_tune
// applies) on a caller's table of radiance samples, table[p][k] (3 doubles) being sample k of
// pixel p, k < budget: each phase's persistent launch is replaced by a gather of the phase's
// slots from the table (k_gather_table).  The pixels form a grid `width` columns wide
// (k_adapt_plan's neighbourhoods).  Out: the pixel statistics ([npix][3] doubles, samples,
// conv), k_resolve's output (rgb, spp_out), and asked[p * budget + k], how often the phases asked
// for each (pixel, sample), saturated at 255.
extern "C" int rtx_internal_adaptive_replay(rtx_scene* sc, const double* table, int64_t npix, int32_t width,
                                            int32_t budget, int32_t min_spp, double rel, double* sum, double* mean,
                                            double* m2, int32_t* samples, uint8_t* conv, double* rgb, int32_t* spp_out,
                                            uint8_t* asked) {
  if (!sc || !table || !rgb || !asked) return fail(RTX_ERR_INVALID, "NULL argument");
  if (npix < 1 || width < 1 || budget < 1 || npix * (int64_t)budget > (1ll << 24))
    return fail(RTX_ERR_INVALID, "adaptive replay: bad table size");
  HIPC(hipSetDevice(sc->device));
  hipStream_t s = sc->stream;
  const size_t entries = (size_t)npix * budget;
  DevBuf d_table, d_asked, d_bad, d_rgb, d_spp;
  int rc;
  if ((rc = d_table.reserve(entries * 3 * sizeof(double)))) return rc;
  if ((rc = d_asked.reserve(entries * sizeof(uint32_t)))) return rc;
  if ((rc = d_bad.reserve(sizeof(unsigned long long)))) return rc;
  if ((rc = d_rgb.reserve(npix * 3 * sizeof(double)))) return rc;
  if ((rc = d_spp.reserve(npix * sizeof(int32_t)))) return rc;
  HIPC(hipMemcpy(d_table.p, table, entries * 3 * sizeof(double), hipMemcpyHostToDevice));
  HIPC(hipMemset(d_asked.p, 0, entries * sizeof(uint32_t)));
  HIPC(hipMemset(d_bad.p, 0, sizeof(unsigned long long)));
  if ((rc = sc->px_sum.reserve(npix * 3 * sizeof(double)))) return rc;
  if ((rc = sc->px_mean.reserve(npix * 3 * sizeof(double)))) return rc;
  if ((rc = sc->px_m2.reserve(npix * 3 * sizeof(double)))) return rc;
  if ((rc = sc->px_samples.reserve(npix * sizeof(int32_t)))) return rc;
  if ((rc = sc->px_conv.reserve(npix))) return rc;
  if ((rc = sc->counters.reserve(kCounterWords * sizeof(unsigned long long)))) return rc;
  const PixelSoA px{sc->px_sum.as<double>(), sc->px_mean.as<double>(), sc->px_m2.as<double>(),
                    sc->px_samples.as<int32_t>(), sc->px_conv.as<uint8_t>()};
  {
    const int64_t n = std::max<int64_t>(npix, kCounterWords);
    hipLaunchKernelGGL(k_frame_init, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, px, npix, 1,
                       sc->counters.as<unsigned long long>(), kCounterWords);
    HIPC(hipGetLastError());
  }
  rtx_render_params prm{};
  prm.spp = budget, prm.adaptive = 1, prm.min_spp = min_spp, prm.rel_threshold = rel;
  prm.mode = RTX_MODE_PERSISTENT;
  RenderArgs A{};
  A.S = sc->S;
  A.npix = npix;
  A.map = PixelMap{};
  A.map.W = A.map.w = width;
  A.map.H = A.map.h = (int32_t)((npix + width - 1) / width);
  set_map_div(A.map);
  A.conv = px.conv;
  A.L = sc->lbuf.as<double>();
  A.counters = sc->counters.as<unsigned long long>();
  Launch L{sc, s, sc->stack_parity, false, false};
  uint64_t hot_launches = 0;
  rc = render_adaptive(
      sc, L, A, &prm, px, budget, 0.0, s, [](hipStream_t) -> int { return RTX_OK; }, hot_launches,
      [](int, int64_t, const uint32_t*) -> int { return RTX_OK; },
      [&](int g, const Launch&, const RenderArgs& Ag, unsigned long long*, uint64_t nslots) -> int {
        if (nslots == 0) return RTX_OK;
        hipLaunchKernelGGL(k_gather_table, dim3((unsigned)((nslots + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           d_table.as<double>(), npix, budget, Ag.L, nslots, g == 1 ? (uint32_t)Ag.K : 0u,
                           sc->aw.smap.as<uint2>(), d_asked.as<uint32_t>(), d_bad.as<unsigned long long>());
        HIPC(hipGetLastError());
        return RTX_OK;
      });
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  hipLaunchKernelGGL(k_resolve, dim3((unsigned)((npix + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, px, npix, 0, budget,
                     d_rgb.as<double>(), d_spp.as<int32_t>());
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  unsigned long long bad = 0;
  HIPC(hipMemcpy(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
  if (bad) return fail(RTX_ERR_INVALID, "adaptive replay: " + std::to_string(bad) + " slots outside the table");
  if ((rc = read_pixels(px, npix, sum, mean, m2, samples, conv))) return rc;
  HIPC(hipMemcpy(rgb, d_rgb.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (spp_out) HIPC(hipMemcpy(spp_out, d_spp.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<uint32_t> h(entries);
  HIPC(hipMemcpy(h.data(), d_asked.p, entries * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < entries; i++) asked[i] = (uint8_t)std::min<uint32_t>(h[i], 255u);
  return RTX_OK;
}

// Test hook (not in rtx.h): a caller's table of radiance samples (table[p][k], 3 doubles, k <
// budget) fed in uniform groups of groups[0], groups[1], ... samples (they sum to the budget)
// through render_device_impl's own accumulate launches (accumulate_group), then resolved.
//   kind 0 / 1  k_accumulate, adaptive on / off (min_spp, rel), then k_resolve
//   kind 2      k_accumulate_sum: the first group with `first`, running sums after it; resolve -1:
//               k_resolve after the last group, 0 / 1: the last group writes the resolved pixel
//               (sum / (float)samples, or the DefaultSampler's sum / spp) in `bands` bands whose
//               edges are multiples of `align` pixels.  The sums start from NaN: `first` must not
//               read them
//   kind 3      k_accumulate_mk_adaptive: AdaptiveSampler(min_spp, budget - 1, rel), then k_resolve
// Out: the pixel statistics as the kernels left them ([npix][3] doubles, samples, conv) and the
// resolved output (rgb, spp_out).
extern "C" int rtx_internal_accumulate_groups(int device, int32_t kind, const double* table, int64_t npix,
                                              int32_t budget, const int32_t* groups, int32_t n_groups, int32_t bands,
                                              int64_t align, int32_t min_spp, double rel, int32_t resolve,
                                              double* sum, double* mean, double* m2, int32_t* samples, uint8_t* conv,
                                              double* rgb, int32_t* spp_out) {
  if (!table || !groups || !rgb) return fail(RTX_ERR_INVALID, "NULL argument");
  if (kind < 0 || kind > 3 || npix < 1 || budget < 1 || n_groups < 1 || bands < 1 || align < 1 || resolve < -1 ||
      resolve > 1 || npix * (int64_t)budget > (1ll << 24))
    return fail(RTX_ERR_INVALID, "accumulate groups: bad arguments");
  int64_t total = 0;
  int kmax = 0;
  for (int i = 0; i < n_groups; i++) {
    if (groups[i] < 1) return fail(RTX_ERR_INVALID, "accumulate groups: empty group");
    total += groups[i], kmax = std::max(kmax, groups[i]);
  }
  if (total != budget) return fail(RTX_ERR_INVALID, "accumulate groups: the groups do not sum to the budget");
  HIPC(hipSetDevice(device));
  DevBuf b_sum, b_mean, b_m2, b_samples, b_conv, b_L, b_rgb, b_spp;
  int rc;
  for (DevBuf* b : {&b_sum, &b_mean, &b_m2, &b_rgb})
    if ((rc = b->reserve(npix * 3 * sizeof(double)))) return rc;
  if ((rc = b_samples.reserve(npix * sizeof(int32_t))) || (rc = b_spp.reserve(npix * sizeof(int32_t)))) return rc;
  if ((rc = b_conv.reserve(npix)) || (rc = b_L.reserve((size_t)npix * kmax * 3 * sizeof(double)))) return rc;
  const int fill = kind == 2 ? 0xFF : 0;  // (0xFF bytes: NaN sums, count -1, which `first` must not read)
  for (DevBuf* b : {&b_sum, &b_mean, &b_m2, &b_samples}) HIPC(hipMemset(b->p, fill, b->n));
  HIPC(hipMemset(b_conv.p, 0, b_conv.n));
  HIPC(hipMemset(b_rgb.p, 0xFF, b_rgb.n));
  HIPC(hipMemset(b_spp.p, 0xFF, b_spp.n));
  const PixelSoA px{b_sum.as<double>(), b_mean.as<double>(), b_m2.as<double>(), b_samples.as<int32_t>(),
                    b_conv.as<uint8_t>()};
  hipStream_t s = nullptr;
  std::vector<double> h;
  bool resolved = false;
  for (int i = 0, s0 = 0; i < n_groups; s0 += groups[i], i++) {
    const int K = groups[i];
    h.resize((size_t)npix * K * 3);
    for (int64_t p = 0; p < npix; p++)
      std::memcpy(h.data() + (size_t)p * K * 3, table + ((size_t)p * budget + s0) * 3, (size_t)K * 3 * sizeof(double));
    HIPC(hipMemcpy(b_L.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    const bool last = i == n_groups - 1;
    GroupAcc ga{kind == 3 ? kAccMkAdaptive : kind == 2 ? kAccSum : kAccRecord, kind == 0 ? 1 : 0, min_spp,
                kind == 3 ? budget - 1 : budget, rel};
    ga.first = s0 == 0;
    if (kind == 2 && last && resolve >= 0) {
      ga.out = AccOut{b_rgb.as<double>(), b_spp.as<int32_t>(), resolve, budget};
      ga.bands = bands, ga.align = align;
      resolved = true;
    }
    if ((rc = accumulate_group(s, px, b_L.as<double>(), npix, K, ga, [](int, int64_t, int64_t) -> int { return RTX_OK; })))
      return rc;
    HIPC(hipStreamSynchronize(s));  // (b_L is rewritten for the next group)
  }
  if (!resolved) {
    hipLaunchKernelGGL(k_resolve, dim3((unsigned)((npix + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, px, npix,
                       kind == 3 ? 2 : 0, budget, b_rgb.as<double>(), b_spp.as<int32_t>());
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
  }
  if ((rc = read_pixels(px, npix, sum, mean, m2, samples, conv))) return rc;
  HIPC(hipMemcpy(rgb, b_rgb.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (spp_out) HIPC(hipMemcpy(spp_out, b_spp.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RTX_OK;
}

// Test hook (not in rtx.h): the launch-constant division of the kernels (FastDiv, the slot ->
// pixel and pixel -> row maps) on the host: out[i] = n[i] / d for i < cnt.
extern "C" int rtx_internal_fastdiv(uint32_t d, const uint32_t* n, int64_t cnt, uint32_t* out) {
  if ((!n || !out) && cnt > 0) return fail(RTX_ERR_INVALID, "NULL argument");
  if (d == 0) return fail(RTX_ERR_INVALID, "division by zero");
  const FastDiv f = make_fastdiv(d);
  for (int64_t i = 0; i < cnt; i++) out[i] = f.div(n[i]);
  return RTX_OK;
}

// Test hook (not in rtx.h): the image rows of stripe `index` of `count` (stripe_rows-row
// interleaved stripes) in the order the render writes them, through the same PixelMap the
// kernels use (subset_pixels, PixelMap::xy): rows[0 .. *nrows).  No device needed.
extern "C" int rtx_internal_stripe_rows(int32_t width, int32_t height, int32_t stripe_rows, int32_t index,
                                        int32_t count, int32_t* rows, int64_t* nrows) {
  if (!rows || !nrows) return fail(RTX_ERR_INVALID, "NULL argument");
  rtx_camera cam{};
  cam.image_width = width, cam.image_height = height;
  rtx_render_params prm{};
  prm.stripe_rows = stripe_rows, prm.stripe_index = index, prm.stripe_count = count;
  PixelMap m;
  std::string err;
  const int64_t n = subset_pixels(&cam, &prm, m, err);
  if (n < 0) return fail(RTX_ERR_INVALID, err);
  *nrows = m.h;
  for (int r = 0; r < m.h; r++) {
    int x, y;
    m.xy((uint32_t)r * (uint32_t)m.w, x, y);
    rows[r] = y;
  }
  return RTX_OK;
}

// Test hook (not in rtx.h): how many adaptive renders of this process sent their output to the
// host early (while phases still ran; render_device_impl `early`), and how many pixels the
// device patched afterwards (k_patch_host), summed over them.
extern "C" int rtx_internal_early_output_stats(long long* outputs, long long* patched) {
  if (!outputs || !patched) return fail(RTX_ERR_INVALID, "NULL argument");
  *outputs = g_early_outputs.load(), *patched = g_early_patched.load();
  return RTX_OK;
}

// Test hook (not in rtx.h): the persistent kernel's LDS layout (persist_lds) for a traversal
// stack of stack_slots entries per lane and a schedule (park: 0 plain, 1 PARK with the
// leaf-step walk, 2 PARK with the speculative walk; + 8: an adaptive phase launch, with its
// block-shared slot chunks):
// out[0..5] = byte offsets of the stack, throughput, hit point, leaf queue, block-wide region
// and the block's LDS size; out[6..9] = the first four regions' bytes per lane (entries x
// element size; they are lane-interleaved with stride kBlock), out[10] = the block-wide region's
// bytes (the chunk words).  tests/test_capi_exports.py checks that the regions are disjoint and
// inside the block's LDS for every stack size the host can choose.
extern "C" int rtx_internal_lds_layout(int stack_slots, int park, uint32_t* out) {
  const int block_kind = (park & 8) ? 1 : 0;
  if ((park & ~11) || stack_slots < 1 || stack_slots > 65 || (park & 3) > 2 || !out)
    return fail(RTX_ERR_INVALID, "bad argument");
  park &= 3;
  const bool spec = spec_walk(park, true, false);
  const PersistLds l = persist_lds(stack_slots, spec, block_kind);
  const uint32_t v[11] = {l.stack, l.thr, l.hitp, l.leafq, l.block, l.end, (uint32_t)stack_slots * (spec ? 2u : 4u),
                          24u, 24u, spec ? kLeafQueue * 4u : 0u, block_region_bytes(block_kind)};
  std::memcpy(out, v, sizeof v);
  return RTX_OK;
}

// Test hook (not in rtx.h): the host-side traversal plan rtx_scene_create makes for `desc`
// (plan_fast_tree, rtx_scene_plan.cc: the routine rtx_scene_create's plan_scene runs), without a device.
// info[0..9] = stack_parity (-1: the tree is deeper than 62 levels and rtx_scene_create refuses
// it), depth, fast_ok, stack_fast, fast_need, n_f4, n_global, global[0], global[1], tree_kind.
// n_global counts the primitives the fast tree was built without, also when fast_ok is 0 (the
// scene then serves fast requests with the parity walk and uses neither tree nor globals).
// f4_out (may be null: a size query) receives the first min(n_f4, f4_cap) F4Nodes, 128 bytes
// each (rtx_device.h); they are built whenever the reference-layout root is internal and the
// depth is accepted, so a tree that needs more than 64 stack entries can still be inspected.
extern "C" int rtx_internal_fast_tree(const rtx_scene_desc* desc, int32_t* info, void* f4_out, int64_t f4_cap) {
  if (!desc || !info) return fail(RTX_ERR_INVALID, "NULL argument");
  if (desc->n_prims < 0 || desc->n_nodes < 0 || (desc->n_prims > 0 && !desc->prims))
    return fail(RTX_ERR_INVALID, "bad scene description");
  if (desc->n_nodes > 0 && !desc->nodes) return fail(RTX_ERR_INVALID, "nodes is NULL");
  for (int64_t i = 0; i < desc->n_prims; i++)
    if (desc->prims[i].kind < RTX_PRIM_SPHERE || desc->prims[i].kind > RTX_PRIM_YZ_RECT)
      return fail(RTX_ERR_INVALID, "bad primitive kind");
  if (const char* why = rtxplan::bad_nodes(desc)) return fail(RTX_ERR_INVALID, why);
  rtxplan::FastPlan p;
  rtxplan::plan_fast_tree(desc, p);
  const int32_t v[10] = {p.stack_parity, p.depth, p.fast_ok ? 1 : 0, p.stack_fast, p.fast_need, (int32_t)p.f4.size(),
                         p.n_global, p.global[0], p.global[1], p.tree_kind};
  std::memcpy(info, v, sizeof v);
  if (f4_out && f4_cap > 0)
    std::memcpy(f4_out, p.f4.data(), (size_t)std::min<int64_t>(f4_cap, (int64_t)p.f4.size()) * sizeof(F4Node));
  return RTX_OK;
}

namespace {

// Which persistent fast schedule suits this scene: the PARK kernel wins where a few lanes
// walk long after the rest of their wave (dense meshes: the bunny, +14..18 %) and loses where
// shading dominates (sphere scenes, -5..-10 %), see DESIGN.md.  Both produce identical
// results, so the choice is timing only: the first persistent fast render of a scene renders
// a centre tile of 1/16 of its pixels with each kernel (twice each; the faster second run
// counts) and keeps the one with the higher segment rate for the scene.
// The timing renders run on the caller's stream `s`, so they are ordered after any render
// still queued there: they share the scene's scratch buffers (pixel state, Lbuf, counters).
int time_park_schedule(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, hipStream_t s) {
  rtx_render_params q = *prm;
  q.stripe_rows = q.stripe_index = q.stripe_count = 0;
  q.w = std::max(1, cam->image_width / 4), q.h = std::max(1, cam->image_height / 4);
  q.x0 = (cam->image_width - q.w) / 2, q.y0 = (cam->image_height - q.h) / 2;
  q.flags = prm->flags & ~(RTX_FLAG_COUNT | RTX_FLAG_PARK | RTX_FLAG_NO_PARK | RTX_FLAG_GENERIC);
  int rc;
  if ((rc = sc->calib_rgb.reserve((size_t)q.w * q.h * 3 * sizeof(double)))) return rc;
  double rate[2] = {0, 0};
  for (int rep = 0; rep < 2; rep++)
    for (int k = 0; k < 2; k++) {
      rtx_render_params r = q;
      r.flags |= k ? RTX_FLAG_PARK : RTX_FLAG_NO_PARK;
      rtx_stats st{};
      if ((rc = rtx_render_device(sc, cam, &r, sc->calib_rgb.as<double>(), nullptr, &st, s))) return rc;
      rate[k] = st.hot_kernel_ms > 0 ? (double)st.rays_total / st.hot_kernel_ms : 0.0;
    }
  sc->park = rate[1] > 1.02 * rate[0] ? 1 : 0;
  return RTX_OK;
}

}  // namespace
