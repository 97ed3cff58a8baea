// Host-side planning helpers of the MSM that carry no device code (also compiled by tests/plan_harness.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include "../../include/icicle_hip.h"

namespace icicle_hip {

  constexpr int MSM_MAX_GROUPS = 16;

  // Window groups of the pipelined schedule (msm_impl.hpp): `tw` windows cut into at most `want` groups, group 0 holding
  // the HIGHEST windows. Group g = [glo[g], ghi[g]); the end groups are half as wide as the inner ones (a short first
  // group lets accumulation start early, a short last one leaves little to reduce at the end). Returns the group count.
  static inline int msm_window_groups(int tw, int want, int* glo, int* ghi)
  {
    int NG = std::max(1, std::min(std::min(want, MSM_MAX_GROUPS), tw / 2));
    if (tw < 4) NG = 1;
    const double unit = (double)tw / (NG <= 2 ? NG : NG - 1);
    double acc = 0;
    int hi = tw;
    for (int g = 0; g < NG; g++) {
      acc += (NG <= 2 || (g > 0 && g < NG - 1)) ? unit : unit / 2;
      int lo = g == NG - 1 ? 0 : std::max(0, tw - (int)(acc + 0.5));
      lo = std::min(lo, hi - 1);
      if (g < NG - 1) lo = std::max(lo, NG - 1 - g); // every later group keeps at least one window
      glo[g] = lo, ghi[g] = hi;
      hi = lo;
    }
    return NG;
  }

  constexpr int MSM_DEFAULT_GROUPS = 1; // window groups of the pipelined schedule (msm_impl.hpp msm_run_pipelined); ICICLE_HIP_MSM_GROUPS overrides
  struct MsmPlan {
    int bits;    // scalar bits considered
    int c;       // window bits (of the widest windows)
    int nwin;    // total windows W = ceil((bits+1)/c)   [mixed plan: chosen W, sum of the widths = bits]
    int pf;      // precompute factor
    int wpf;     // windows per precomputed base = target windows actually accumulated
    uint32_t nb; // buckets per window = 2^(c-1) (array stride of every per-bucket table)
    uint32_t seg; // bucket-accumulation segment size: a bucket with more points is split across threads
    // Mixed window widths (round 5): windows [0, n_lo) are c - 1 bits wide and use the first nb / 2 buckets of their slot,
    // windows [n_lo, nwin) are c bits wide; n_lo = 0 is the uniform plan of rounds 1-4. With `negate` a scalar whose top bit
    // is set is replaced by r - s and its point negated (the reference's own trick, cpu_msm.hpp:276-277), so scalars stay
    // below 2^(bits-1) and the widths only have to add up to `bits`: 254 bits = 10 x 21 + 2 x 22, twelve windows instead of
    // the thirteen of c = 20 (-7.7 % mixed additions) for 2.15 x the buckets (uniform c = 22: 3.7 x, measured a wash).
    int n_lo = 0;
    bool negate = false;
    int width(int w) const { return w < n_lo ? c - 1 : c; }
    int offset(int w) const { return w < n_lo ? w * (c - 1) : n_lo * (c - 1) + (w - n_lo) * c; } // bit offset of window w
    uint32_t nb_of(int w) const { return w < n_lo ? nb / 2 : nb; }
    size_t buckets_used() const { return (size_t)n_lo * (nb / 2) + (size_t)(nwin - n_lo) * nb; }
  };

  // force_windows: 0 = the cost model decides; W > 0 = W windows whose widths add up to the scalar bits (tests, A/B:
  // MSMConfig.ext "hip_msm_windows"); -1 = uniform widths only (callers that fix config.c for several sub-calls)
  static MsmPlan make_plan(int n, int scalar_bits, const icicle_msm_config_t& cfg, int force_windows = 0)
  {
    MsmPlan p;
    p.bits = (cfg.bitsize > 0 && cfg.bitsize < scalar_bits) ? cfg.bitsize : scalar_bits;
    p.pf = std::max(1, cfg.precompute_factor);
    int c = cfg.c;
    // A precomputed base table fixes the doubling shift c * wpf, so msm_precompute_bases(nof_bases) and msm(msm_size)
    // must agree on c. Like the reference (cpu_msm.hpp:466 vs :207, get_optimal_c :103-119) both sides derive it from the
    // size of ONE MSM, the scalar bits and precompute_factor -- and from nothing else: with precompute_factor > 1 the
    // choice ignores batch_size (the two calls rarely carry the same one: the Rust suite precomputes shared bases with
    // batch_size 1 and then runs batches of 1, 3 and 16 on the table, wrappers/rust/icicle-core/src/msm/tests.rs:96-134).
    // msm_precompute_bases is handed the size of one MSM as nof_bases by both wrappers (msm_impl.hpp msm_precompute_run), and
    // msm() on a table this process wrote takes c from the table registry (common.h) before it gets here. Rounds 1-3 used a fixed c = 16 here, which made every MSM from 2^20 up
    // SLOWER with a table (16 windows against 13); now a table lowers the bucket count per window set by pf and the cost
    // model moves c up with it, as docs/docs/api/cpp/msm.md:155-201 describes. Pass config.c on both calls to override.
    const bool table = p.pf > 1;
    if (c <= 0) {
      // minimise  (#mixed adds) + (bucket-reduction work). Fitted to a measured sweep (profiles/r03_msm_csweep.txt):
      //  * a window size whose TOP window holds only 1-3 scalar bits is never chosen: that window has a handful of
      //    buckets with n/4 points each, i.e. one more window of mixed adds for nothing plus the whole overflow machinery
      //    (c = 14, 18, 21 for 254-bit scalars: 2^20 4.7 / 4.6 ms against 2.9 ms at c = 17; 2^26 98 against 71 ms);
      //  * n >= 2^16: with fewer than ~2.5 waves of bucket threads per SIMD the accumulation runs below its issue rate,
      //    which favours MORE buckets than the add count alone suggests, and a bucket costs 2 (below 2^22) to 4 add-
      //    equivalents in the reduction (2^16: c 13 -> 15, 2.10 -> 1.74 ms; 2^18: 2.67 -> 2.15; 2^20: 15 -> 17, 3.4 -> 2.9);
      //  * below 2^16 the latency of the reduction and of the window combine dominates: per bucket: ~2 complete adds
      //    (14 muls each) vs 10 muls per mixed add, weighted 8 for their poor parallelism (round 1's fit, still the best).
      // (a batch runs as ONE launch sequence with batch x the bucket threads and batch x the reduction work: round 1's
      //  weights stay the better fit there -- 16 x 2^16: 3.5 ms against 4.5 ms with the single-MSM fit)
      const bool mid = n >= (1 << 16) && (table || std::max(1, cfg.batch_size) == 1);
      // A single small MSM of full-width scalars is a chain of latencies, and since the bucket reduction runs four lanes per column
      // (round 6, msm_impl.hpp k_reduce_wave_quad) a bucket costs little: what counts is the length of the accumulation chains
      // (n / 2^(c-1) mixed additions per bucket) and the window count. Measured sweeps (profiles/r06_small_msm_c_sweep.txt): up to 2^12
      // terms c = 8 (32 windows; BN254 2^10 1.23 -> 0.89 ms, BLS12-381 2^11 2.14 -> 1.58), above c = 15 (17 windows of a 254-bit scalar;
      // BN254 2^15 1.48 -> 1.09 ms) -- or the next c whose top window is not a stub (BLS12-381: 16; 2^15 2.74 -> 2.05 ms).
      int small_c = 0;
      // (up to 2^18 terms: from 2^16 the fit below picks 15 for 253 / 254-bit scalars itself, but 13 / 14 for 255-bit ones where 15 leaves a one-bit
      //  top window -- BLS12-381 2^16 2.81 ms against 2.14 at c = 16, 2^17 2.94 against 2.29)
      if (!table && std::max(1, cfg.batch_size) == 1 && n < (1 << 18) && p.bits >= 200) {
        small_c = n <= (1 << 12) ? 8 : 15;
        for (;; small_c++) {
          const int w = (p.bits + 1 + small_c - 1) / small_c;
          if (!(w > 1 && p.bits + 1 - small_c * (w - 1) <= 3)) break;
        }
      }
      double best = 1e300;
      for (int cc = (small_c ? small_c : 2); cc <= (small_c ? small_c : 21); cc++) {
        const int w = (p.bits + 1 + cc - 1) / cc;
        const int wpf = (w + p.pf - 1) / p.pf;
        if (w > 1 && p.bits + 1 - cc * (w - 1) <= 3 && p.bits > 8) continue; // tiny top window
        // batches of small MSMs: the one-level sort (c <= 11) beats the two-level one by far while the windows are small
        // (128 x 2^17: c = 11 29.2 ms, c = 12 / 13 36.4 / 34.8; 1024 x 2^12: c = 12 77 ms against 16) -- profiles/r03_notes.md 11
        if (!table && cfg.batch_size > 1 && n <= (1 << 17) && cc > 11) continue;
        const double nbk = (double)wpf * (double)(1u << (cc - 1));
        double cost;
        if (mid) {
          const double occupancy = std::max(1.0, 2.5 * 65536.0 / nbk); // bucket threads per SIMD lane slot
          // (below 2^22 the reduction is latency-, not throughput-bound -- but with a base table there are few bucket sets, and a
          //  wider window buys them at the full price: fitted to profiles/r04_precompute_csweep.txt, e.g. 2^18, pf 8: c = 17 1.96 ms,
          //  c = 19 2.29 ms)
          cost = (double)w * n * occupancy + ((table || n >= (1 << 22)) ? 4.0 : 2.0) * nbk;
        } else {
          cost = (double)w * n + 8.0 * nbk;
        }
        if (cost < best) {
          best = cost;
          c = cc;
        }
      }
    }
    // two-level sort: 2^hb partitions (pass A, hb <= 10) x 2^lb bins (pass B, lb <= 11). The model above stops at 21: a caller-set
    // 22 runs (12 windows of a 254-bit scalar instead of 13, four times the buckets of c = 20) and was measured slower at 2^26
    // (profiles/r04_msm_csweep.txt)
    c = std::min(22, std::max(2, c));
    p.c = c;
    p.nwin = (p.bits + 1 + c - 1) / c;
    p.wpf = (p.nwin + p.pf - 1) / p.pf;
    p.nb = 1u << (c - 1);
    // ---- mixed widths: W windows, the top x of them one bit wider, widths adding up to the scalar bits exactly. Needs the
    // negation trick, i.e. full-width scalars (a chopped scalar has no top bit to test, cpu_msm.hpp:276), no base table (its
    // doubling shift is c * wpf) and the two-level sort (c - 1 >= 12). The cost model compares it with the best uniform plan
    // at the same weights: it wins from ~2^25 terms up, where a window of mixed additions outweighs twice the buckets.
    if (cfg.c <= 0 && p.pf == 1 && p.bits == scalar_bits && std::max(1, cfg.batch_size) == 1 && (force_windows > 0 || (force_windows == 0 && n >= (1 << 23)))) {
      auto uniform_cost = [&](int w, double nbk) {
        const double occupancy = std::max(1.0, 2.5 * 65536.0 / nbk);
        return (double)w * n * occupancy + 4.0 * nbk;
      };
      int bestW = 0;
      double best = force_windows > 0 ? 1e300 : 0.995 * uniform_cost(p.nwin, (double)p.nwin * p.nb);
      for (int W = (force_windows > 0 ? force_windows : 2); W <= (force_windows > 0 ? force_windows : 40); W++) {
        const int clo = p.bits / W, x = p.bits - clo * W; // x windows of clo + 1 bits, W - x of clo bits
        if (x == 0 || clo + 1 > 22 || clo < (force_windows > 0 ? 2 : 12)) continue;
        const double nbk = (double)(W - x) * (double)(1u << (clo - 1)) + (double)x * (double)(1u << clo);
        const double cost = force_windows > 0 ? 0.0 : uniform_cost(W, nbk);
        if (cost < best) best = cost, bestW = W;
      }
      if (bestW > 0) {
        const int clo = p.bits / bestW, x = p.bits - clo * bestW;
        p.c = clo + 1;
        p.nwin = p.wpf = bestW;
        p.n_lo = bestW - x;
        p.negate = true;
        p.nb = 1u << (p.c - 1);
      }
    }
    {
      // points per bucket: the nwin windows of a scalar land in wpf bucket sets. (Rounds 1-3 had one more factor pf here: with
      // a base table the segments came out pf times too long, and the handful of buckets that take the whole short top window
      // -- n / 2^(top bits - 1) points each -- were walked by a few threads in chains of thousands of additions: pf = 8, c = 19
      // at 2^24 took 49.9 ms against 19.9 ms at c = 20, profiles/r04_precompute_sweep.txt.)
      const double avg = (double)n * ((double)p.nwin / p.wpf) / (double)(p.n_lo > 0 ? p.nb / 2 : p.nb); // (of the narrow windows)
      uint32_t sgm = 64;
      while ((double)sgm < 2.0 * avg)
        sgm <<= 1;
      p.seg = sgm;
    }
    return p;
  }

  // ---- constants the kernels and the launch plans below share (what each is for: at its kernels in msm_impl.hpp) ----
  constexpr int SORT_EPT = 16;                          // tile sort: elements per thread per tile
  constexpr uint32_t SORT_TS = 1024 * SORT_EPT;         // tile size with 1024 threads
  constexpr uint32_t SCAN_CHUNK = 8192;                 // k_scan_*: 1024 threads x 8 consecutive elements
  constexpr uint32_t CHUNKB_LOG = 17;                   // pass B, sub-chunk route: elements per block = 2^17
  constexpr uint32_t PASSB_OWN_MAX_DEFAULT = 1u << 18;  // pass B, owned route: largest partition one block sorts whole
  constexpr uint32_t SZ_BINS = 257;                     // size classes of the size-balanced bucket order
  constexpr uint32_t SZ_CHUNK = 16384;                  // k_bsize_*: buckets per block (1024 threads x 16)
  constexpr int FINAL_WINDOWS_PER_BLOCK = 16;           // k_final: windows per single-wave block
  // LDS bytes of a tile sort over D destinations (msm_impl.hpp tile_lds lays them out)
#if defined(__HIPCC__)
  __host__ __device__
#endif
  static inline size_t tile_lds_bytes(uint32_t D, uint32_t TS = SORT_TS) { return ((size_t)2 * D + TS + TS / 2 + 32) * 4; }

  // ---- environment overrides (A/B knobs). All of them are read ONCE per process, by msm_env_knobs(); the plan functions below
  // take the struct as an argument so that a host test can force any knob without touching the environment. ----
  struct MsmKnobs {
    int windows = 0;                     // ICICLE_HIP_MSM_WINDOWS: W > 0 forces W mixed-width windows, -1 = uniform only, 0 = the cost model
    bool hb_set = false;                 // ICICLE_HIP_MSM_HB: high key bits of the two-level sort (clamped into the sort's range)
    int hb = 0;
    bool mrow_set = false;               // ICICLE_HIP_MSM_MROW: cap of the bucket reduction's rows per lane
    int mrow = 0;
    int groups = MSM_DEFAULT_GROUPS;     // ICICLE_HIP_MSM_GROUPS: window groups of the pipelined schedule
    bool coresident = true;              // ICICLE_HIP_MSM_CORESIDENT=0: no co-resident sort beside the accumulation
    bool acc_waves_set = false;          // ICICLE_HIP_MSM_ACC_WAVES: waves per SIMD k_accumulate is compiled for
    int acc_waves = 0;
    bool reduce_balance = false;         // ICICLE_HIP_MSM_REDUCE_BALANCE=1: half the rows per lane for the narrow windows of a mixed plan
    bool reduce_small = true;            // ICICLE_HIP_MSM_REDUCE_SMALL=0: no k_reduce_small
    bool reduce_quad = true;             // ICICLE_HIP_MSM_REDUCE_QUAD=0: no four-lane bucket reduction
    bool reduce_signed = true;           // ICICLE_HIP_MSM_REDUCE_SIGNED=0: the one-lane bucket reduction adds with EC::add, not EC::add_signed
    bool host_combine = true;            // ICICLE_HIP_MSM_HOST_COMBINE=0: the window combine always on the device
    bool batch_horner = true;            // ICICLE_HIP_MSM_BATCH_HORNER=0: no k_final_horner
  };
  inline const MsmKnobs& msm_env_knobs()
  {
    static const MsmKnobs knobs = [] {
      MsmKnobs k;
      auto on_unless_0 = [](const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); };
      if (const char* e = getenv("ICICLE_HIP_MSM_WINDOWS")) k.windows = atoi(e);
      if (const char* e = getenv("ICICLE_HIP_MSM_HB")) k.hb_set = true, k.hb = atoi(e);
      if (const char* e = getenv("ICICLE_HIP_MSM_MROW")) k.mrow_set = true, k.mrow = std::max(1, atoi(e));
      if (const char* e = getenv("ICICLE_HIP_MSM_GROUPS")) k.groups = atoi(e);
      k.coresident = on_unless_0("ICICLE_HIP_MSM_CORESIDENT");
      if (const char* e = getenv("ICICLE_HIP_MSM_ACC_WAVES")) k.acc_waves_set = true, k.acc_waves = atoi(e);
      if (const char* e = getenv("ICICLE_HIP_MSM_REDUCE_BALANCE")) k.reduce_balance = atoi(e) != 0;
      k.reduce_small = on_unless_0("ICICLE_HIP_MSM_REDUCE_SMALL");
      k.reduce_quad = on_unless_0("ICICLE_HIP_MSM_REDUCE_QUAD");
      k.reduce_signed = on_unless_0("ICICLE_HIP_MSM_REDUCE_SIGNED");
      k.host_combine = on_unless_0("ICICLE_HIP_MSM_HOST_COMBINE");
      k.batch_horner = on_unless_0("ICICLE_HIP_MSM_BATCH_HORNER");
      return k;
    }();
    return knobs;
  }

  // ---- two-level counting sort (msm_impl.hpp section 2+3) ----
  struct SortPlan {
    int hb, lb;       // high / low bucket-key bits, hb + lb = c - 1
    int jb;           // bits for the precompute index j
    int chunk_log;    // scalars per pass-A block = 2^chunk_log
    int nblk;         // pass-A blocks
  };
  // The sort geometry of n scalars in windows of c bits with precompute factor pf. false: the shape does not fit the sort
  // (the caller answers ICICLE_INVALID_ARGUMENT).
  static inline bool msm_sort_plan(int n, int c, int pf, const MsmKnobs& kn, SortPlan* sp)
  {
    const int kb = c - 1;
    // each tile-sorted pass ranks into <= 1024 destinations (one per thread of the block); small
    // windows (kb <= 10) need a single level: pass A already produces the bucket lists
    int hb = kb <= 10 ? kb : (kb + 1) / 2;
    if (kn.hb_set) hb = kn.hb;
    hb = std::max(kb - 11, std::min(std::min(kb, 10), hb)); // pass A: at most 2^10 partitions; pass B: up to 2^11 bins (c = 22)
    if (hb < 0 || hb > 10 || kb - hb > 11) return false;
    sp->hb = hb;
    sp->lb = kb - hb;
    sp->jb = 0;
    while ((1 << sp->jb) < pf)
      sp->jb++;
    int logn = 0;
    while (((size_t)1 << logn) < (size_t)n)
      logn++;
    const int max_chunk = 31 - sp->lb - sp->jb;
    if (max_chunk < 10) return false;
    sp->chunk_log = std::max(10, std::min(max_chunk, std::max(17, logn - 9)));
    if (sp->chunk_log < logn - 9) return false; // would need more than 512 pass-A blocks per window
    sp->nblk = (int)(((size_t)n + ((size_t)1 << sp->chunk_log) - 1) >> sp->chunk_log);
    return true;
  }

  // ---- bucket reduction geometry: a wave owns a chunk of 64*mrow buckets; at most rwl chunks per window (one thread of the
  // per-window kernel each; rwl = ReduceWindowLanes<C>::value), at least 16 rows per lane when the window is big enough to
  // amortise the wave scans ----
  struct MsmReduceGeom {
    uint32_t mrow;      // rows per lane
    uint32_t m;         // buckets per chunk = 64 * mrow ("segment" of the exchange hook)
    uint32_t nseg;      // chunks per window
    uint32_t log_chunk; // ceil(log2(m))
  };
  // Rows per lane: 16 amortise the wave scans; a single mid-size MSM has fewer reduction waves than the chip has SIMDs
  // and is bound by the length of one wave's chain, so there the rows shrink until the waves fill the SIMDs once
  // (2^16, c = 15: 272 waves of 16 rows -> 544 of 8, 1.78 -> 1.59 ms; at 2^20 16 rows already make 960 waves). The rule
  // depends on the window plan only (every shard of a multi-device call derives the same geometry).
  static inline MsmReduceGeom msm_reduce_geom(int batch, int wpf, uint32_t nb, uint32_t rwl, const MsmKnobs& kn)
  {
    uint32_t mrow_cap = 16;
    if (batch == 1 && nb >= 8192) {
      uint32_t need = (uint32_t)(((uint64_t)wpf * nb + 65535) / 65536), p2 = 2;
      while (p2 < need)
        p2 <<= 1;
      mrow_cap = std::min<uint32_t>(16, p2);
    }
    if (kn.mrow_set) mrow_cap = (uint32_t)kn.mrow; // (A/B knob)
    MsmReduceGeom g;
    g.mrow = std::max<uint32_t>(1, std::max<uint32_t>(nb / (64 * rwl), std::min<uint32_t>(mrow_cap, nb / 64)));
    g.m = 64 * g.mrow;
    g.nseg = std::max<uint32_t>(1, nb / g.m);
    g.log_chunk = 0;
    while ((1u << g.log_chunk) < g.m)
      g.log_chunk++;
    return g;
  }

  // ---- batch folding: BB MSMs of the batch run as ONE launch sequence with BB*wpf windows
  // (wrappers/rust/icicle-core/src/msm/tests.rs:92-254 batches; small MSMs would otherwise leave the
  // GPU idle). BB is bounded by a memory budget -- half of `free_bytes`, at most 48 GiB -- and by the grid.y limit.
  // per_msm_bytes: digits + bucket lists (two copies with a two-level sort) + buckets and their counters + pass-A tables +
  // `staged_base_bytes` (the converted copy of bases that are neither shared nor canonical). proj_bytes = sizeof(Proj).
  // Returns BB, or 0 when a bucket-exchange hook needs the whole batch in one launch group and that exceeds the grid
  // (msm_multi_run checked the limit).
  static inline int msm_batch_fold(const MsmPlan& pl, const SortPlan& sp, int n, size_t proj_bytes, size_t staged_base_bytes, size_t free_bytes, int batch, bool has_hook)
  {
    const size_t cap = (size_t)n * pl.pf;
    const size_t per_msm_bytes = (size_t)pl.nwin * n * 4 + (sp.lb == 0 ? 1 : 2) * (size_t)pl.wpf * cap * 4 + (size_t)pl.wpf * pl.nb * (proj_bytes + 12) +
                                 (size_t)pl.wpf * ((size_t)1 << sp.hb) * sp.nblk * 8 + staged_base_bytes;
    const size_t budget = std::min((size_t)48 << 30, free_bytes / 2);
    int BB = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, budget / std::max<size_t>(per_msm_bytes, 1)));
    BB = std::min(BB, std::max(1, 60000 / pl.wpf));
    if (has_hook && BB < batch) {
      BB = batch;
      if ((size_t)BB * pl.wpf > 60000) return 0;
    }
    return BB;
  }

  // ---- bucket reduction of one window group: THE place where its kernels are decided (msm_impl.hpp MsmLaunch::reduce_group
  // launches what this returns). Windows [w0, w0 + nw) of a plan whose windows below n_lo are narrow (half the buckets);
  // chunks [seg_lo, seg_lo + nsegr) of every window (the whole window unless a bucket-exchange hook left this device a slice). ----
  enum class MsmChunkKernel { none, wave_quad, small, wave };
  enum class MsmWindowKernel { none, window_quad, window };
  struct MsmReduceRoute {
    MsmChunkKernel chunk;
    MsmWindowKernel window; // none: the chunk kernel writes the window sums itself
    bool direct;            // ... which it does
    uint32_t nlo_w;         // narrow windows of the group
    // k_reduce_wave_quad: nsq chunks of 16 * mq buckets per window, four lanes per bucket column
    uint32_t nsq, mq;
    // k_reduce_small: 2^lw_log lanes per window, per_wave windows per wave
    uint32_t lw_log, per_wave;
    // k_reduce_wave: one block per chunk; the narrow windows have nseg_lo chunks of 64 * mrow_lo buckets
    size_t nblocks;
    uint32_t mrow_lo, nseg_lo, log_chunk_lo;
    // window kernel: k_reduce_window_quad over wchunks chunks of wchunk_size buckets, or k_reduce_window; wthreads per block
    uint32_t wchunks, wchunk_size, wthreads;
    // what the quad decision compared (0 when it was not reached): additions on the chain x instructions per addition (in
    // hundreds) x rounds of waves on the 1024 SIMDs, four-lane against one-lane
    uint64_t cost_q, cost_s;
  };
  static inline MsmReduceRoute msm_reduce_route(uint32_t nb, int w0, int nw, int n_lo, const MsmReduceGeom& geo, uint32_t seg_lo, uint32_t nsegr, bool has_hook, int NG, int bb, bool quad_ok, uint32_t rwl, const MsmKnobs& kn)
  {
    MsmReduceRoute r{};
    const uint32_t mrow = geo.mrow, nseg = geo.nseg;
    // windows [w0, split) of the group are the narrow windows of a mixed-width plan (half the buckets, nseg_lo chunks), the
    // rest wide; one launch of each kernel serves both (a uniform plan has n_lo = 0: no narrow windows). (bb == 1 whenever n_lo > 0)
    const int split = std::min(std::max(n_lo, w0), w0 + nw);
    r.nlo_w = (uint32_t)(split - w0);
    // narrow windows: half the rows per lane, so that they have as many chunks as the wide ones (see k_reduce_wave)
    // Measured and left OFF (profiles/r06_msm_reduce_balance_ab.txt, same box, BN254 2^26): tail 4.72 / 4.75 ms without, 4.90 / 4.86 ms
    // with -- the extra 1280 waves bring 19 scan additions each, more than the evened-out SIMD load gives back. ICICLE_HIP_MSM_REDUCE_BALANCE=1: on.
    r.mrow_lo = (kn.reduce_balance && r.nlo_w > 0 && mrow >= 2 && !has_hook) ? mrow / 2 : mrow;
    r.nseg_lo = std::max<uint32_t>(1, (nb / 2) / (64 * r.mrow_lo));
    r.log_chunk_lo = r.mrow_lo == mrow ? geo.log_chunk : geo.log_chunk - 1;
    r.nblocks = (size_t)r.nlo_w * r.nseg_lo + (size_t)(nw - r.nlo_w) * nsegr;
    const bool whole_single_chunk = (nseg == 1 && nsegr == 1 && seg_lo == 0); // the one-lane chunk kernel writes the window sums
    auto window_quad_threads = [](uint32_t chunks) { // four lanes per chunk, a power of two
      uint32_t t = 64;
      while (t < 4 * chunks)
        t <<= 1;
      return t;
    };
    // whole small windows: several per wave (k_reduce_small); rows per lane: 8, or 4 for the tiniest windows
    const bool small_path = kn.reduce_small && whole_single_chunk && r.nlo_w == 0 && nb >= 16 && nb <= 512 && nw >= 64;
    // Four lanes per bucket column while the reduction is a latency chain (single MSM, uniform plan, one device): the window kernel
    // whenever a window has at most 64 chunks, the wave kernel when its shorter additions beat the one-lane kernel's 3.5 x fewer
    // lanes -- up to ~2^18 terms; beyond, the reduction is work and the one-lane kernel wins (2^20: 0.56 against 0.43 ms).
    // ICICLE_HIP_MSM_REDUCE_QUAD=0: off (A/B). quad_ok: G1, and the G2 whose point fits the registers four lanes deep (BN254's --
    // BLS12-381's 28-limb Fq2 elements do not).
    bool quad_window = false;
    if (quad_ok && kn.reduce_quad && !has_hook && NG == 1 && bb == 1 && n_lo == 0 && seg_lo == 0 && nsegr == nseg && nb >= 16 && !small_path) {
      quad_window = nseg <= 64 && !whole_single_chunk;
      if (nb <= 65536) {
        // chunks per window so that the waves fill the SIMDs once (a wave past 1024 doubles the time of its SIMD), rows to match
        uint32_t nsq = std::min<uint32_t>(std::min<uint32_t>(64, std::max<uint32_t>(1, 1024 / (uint32_t)nw)), nb / 16);
        const uint32_t mq = (nb + 16 * nsq - 1) / (16 * nsq);
        nsq = (nb + 16 * mq - 1) / (16 * mq);
        r.cost_q = (uint64_t)(2 * mq + 13) * 13 * (((uint64_t)nw * nsq + 1023) / 1024);
        r.cost_s = (uint64_t)(2 * mrow + 19) * 29 * (((uint64_t)nw * nseg + 1023) / 1024);
        if (r.cost_q < r.cost_s) {
          r.chunk = MsmChunkKernel::wave_quad;
          r.nsq = nsq, r.mq = mq;
          r.direct = nsq == 1;
          if (!r.direct) r.window = MsmWindowKernel::window_quad, r.wchunks = nsq, r.wchunk_size = 16 * mq, r.wthreads = window_quad_threads(nsq);
          return r;
        }
      }
    }
    r.direct = whole_single_chunk;
    if (small_path) {
      r.chunk = MsmChunkKernel::small;
      r.lw_log = 2;
      while ((nb >> r.lw_log) > 8 && r.lw_log < 5)
        r.lw_log++;
      r.per_wave = 64u >> r.lw_log;
    } else if (r.nblocks) {
      r.chunk = MsmChunkKernel::wave;
    }
    if (r.direct) return r;
    if (quad_window) {
      r.window = MsmWindowKernel::window_quad, r.wchunks = nseg, r.wchunk_size = 64 * mrow, r.wthreads = window_quad_threads(nseg);
    } else {
      r.window = MsmWindowKernel::window;
      r.wthreads = 64; // power of two (LDS tree), >= the chunks of a window
      while (r.wthreads < std::max(nsegr, r.nlo_w ? r.nseg_lo : 0u) && r.wthreads < rwl)
        r.wthreads <<= 1;
    }
    return r;
  }

  // ---- window combine of a single-group launch sequence ----
  // Host: when the result goes there anyway or the call waits for the stream anyway (msm_impl.hpp MsmLaunch::host_combine says why);
  // single MSMs only. k_final_horner: big batches. Else k_final, one single-wave block per FINAL_WINDOWS_PER_BLOCK windows, and
  // with more than one block per MSM k_final_combine adds their partial sums.
  enum class MsmCombine { host, final_horner, final_only, final_then_combine };
  static inline MsmCombine msm_combine_route(bool results_on_device, bool is_async, int batch, int bb, bool has_hook, int wpf, const MsmKnobs& kn)
  {
    if (kn.host_combine && (!results_on_device || !is_async) && batch == 1 && bb == 1 && !has_hook && wpf <= 64) return MsmCombine::host;
    if (kn.batch_horner && bb >= 64 && wpf >= 2) return MsmCombine::final_horner;
    return wpf > FINAL_WINDOWS_PER_BLOCK ? MsmCombine::final_then_combine : MsmCombine::final_only;
  }

  // ---- the k_accumulate instantiation to launch: waves per SIMD the register allocator must leave room for (3 fits BN254 G1,
  // 157 VGPRs, without spilling; 2 fits BLS12-381 G1 -- 14-limb elements -- and BN254 G2; 1 for BLS12-381 G2), and the padded
  // two-wave form that leaves room for the co-resident sort (9-limb G1 only: co_ok is never set for another curve class).
  // is_g2: the XYZZ point is larger than 256 bytes; limbs: limbs of a base-field element (EC<C>::F::N). ----
  struct MsmAccWaves {
    int minw;
    bool pad;
  };
  static inline MsmAccWaves msm_acc_waves(bool is_g2, size_t xyzz_bytes, int limbs, bool co_ok, const MsmKnobs& kn)
  {
    const int want = kn.acc_waves_set ? kn.acc_waves : (is_g2 ? (xyzz_bytes <= 288 ? 2 : 1) : (limbs <= 9 ? 3 : 2));
    if (is_g2) return {(xyzz_bytes <= 288 && want >= 2) ? 2 : 1, false};
    if (co_ok) return {2, true};
    return {(want == 1 || want == 2 || want == 4) ? want : 3, false};
  }

} // namespace icicle_hip
