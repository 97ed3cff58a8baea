// Host check of the NTT pass plan (icicle_amd/csrc/ntt_plan.h): for every size, every pass's tiles must touch each
// slot of a row exactly once on the way in, and the last pass's natural-order scatter must hit each output once.
// The address formulas are the kernels' (k_ntt_fast / k_ntt_pass_generic / k_big_ntt_pass).
#include "../icicle_amd/csrc/ntt_plan.h"
#include "../icicle_amd/csrc/msm_plan.h"
#include <cstdio>
#include <future>
#include <vector>
#include <algorithm>
using namespace icicle_hip;

// big_elem_bytes = 0: the 31-bit NTT (tile width by k_ntt_fast's rule, at most tmax_cap columns). Otherwise the pass geometry of
// ntt_big.hip, from the function big_ntt_run launches with (ntt_plan.h big_pass_geometry): big_elem_bytes per element in LDS, tiles of at
// most tmax_cap columns, radix16 for goldilocks' four stages per LDS trip. walk = false: the geometry assertions only, no bijection walk.
static int check(int logn, int smax, uint32_t tmax_cap, bool ntt31, uint32_t big_elem_bytes = 0, bool radix16 = false, bool walk = true)
{
  int parts[3], P;
  if (ntt31)
    ntt_split_parts(logn, -1, parts, &P); // the 31-bit NTT's pass lengths (8,9,8 at 2^25)
  else
    split_logn(logn, smax, parts, &P); // ntt_big.hip
  int sum = 0;
  for (int i = 0; i < P; i++)
    sum += parts[i];
  if (sum != logn || P < 1 || P > 3) return 1;
  const uint64_t n = 1ull << logn;
  for (int p = 0; p < P; p++) {
    const uint64_t L = 1ull << parts[p];
    PassDesc pd;
    if (big_elem_bytes) {
      const BigPass bp = big_pass_geometry(parts, P, p, n, /*log_max=*/logn, big_elem_bytes, tmax_cap, radix16);
      pd = bp.pd;
      const int s = parts[p];
      if (bp.tot != L * (uint64_t)pd.T || bp.lds_bytes != (uint64_t)bp.tot * big_elem_bytes) return 50 + p;
      if (bp.lds_bytes > 72 * 1024 || (uint32_t)pd.T > tmax_cap) return 50 + p; // two blocks share a CU's 160 KiB
      if (bp.threads < 64 || bp.threads > 512 || (bp.threads & (bp.threads - 1)) != 0) return 60 + p; // __launch_bounds__(512)
      if (bp.threads % (uint32_t)pd.T != 0) return 60 + p; // the goldilocks store: a thread stays in its column from trip to trip
      // k_big_ntt_pass's stage loops: groups of 16 elements (goldilocks, while four stages remain), then of 4 (two stages), then
      // of 2 (an odd last stage); every element of the tile must belong to exactly one group of each loop that runs
      int q = 0;
      if (radix16)
        for (; q + 3 < s; q += 4)
          if (bp.tot % 16 != 0) return 70 + p;
      for (; q + 1 < s; q += 2)
        if (bp.tot % 4 != 0) return 70 + p;
      if (q < s && bp.tot % 2 != 0) return 70 + p;
      // load and store walk e = tid, tid + blockDim, ...: whole trips (and the store's progression advances once per trip)
      if (bp.tot >= bp.threads && bp.tot % bp.threads != 0) return 80 + p;
    } else {
      const uint64_t epb = L >= 16 ? 16 : L;
      uint32_t tmax = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tmax_cap, 512 * epb / L));
      while (tmax > 1 && 2 * L * (tmax + 1) * 4 > 160 * 1024)
        tmax >>= 1;
      pd = make_pass(parts, P, p, n, /*log_max=*/logn, tmax);
    }
    if (pd.T < 1 || (uint64_t)pd.ntiles * pd.T * L != n) return 10 + p;
    if (!walk) continue;
    std::vector<uint8_t> in(n, 0), out(n, 0);
    for (uint32_t tile = 0; tile < pd.ntiles; tile++) {
      const uint32_t a = tile / pd.tiles_per_a, ct = tile % pd.tiles_per_a;
      const uint64_t in_base = (uint64_t)a * pd.in_base_a + (uint64_t)ct * pd.in_base_ct;
      for (uint64_t k = 0; k < L; k++)
        for (int t = 0; t < pd.T; t++) {
          const uint64_t addr = in_base + k * pd.in_sk + (uint64_t)t * pd.in_st;
          if (addr >= n || in[addr]++) return 20 + p;
          if (pd.is_last) {
            const uint64_t K0 = (pd.pidx <= 1) ? ((uint64_t)ct * pd.T + t) : (((uint64_t)ct * pd.T + t) + (uint64_t)pd.n0 * a);
            const uint64_t o = K0 + k * pd.out_sk;
            if (o >= n || out[o]++) return 30 + p;
          } else {
            const uint64_t c = (uint64_t)ct * pd.T + t;
            if (c / pd.cprime >= (1ull << parts[p + 1])) return 40 + p; // jnext is a digit of the next pass
          }
        }
    }
  }
  return 0;
}

// max_logn: the 31-bit fields (up to 2^27, BabyBear's two-adicity: the 512-row passes from 2^25 up); max_logn_big: ntt_big.hip's fields
// (256-bit: 36-byte LDS elements, tiles of at most 4 columns; goldilocks: 8-byte elements, at most 16 columns, four stages per trip).
// The bijection walk stops at 2^27 (a walk touches every element of every pass); 2^28 gets the geometry assertions.
// Failures: logn * 100 + code (31-bit), + 1000000 (256-bit), + 2000000 (goldilocks).
extern "C" int plan_check(int max_logn, int max_logn_big)
{
  // the three families are independent: one thread each (the walks of the large sizes are the whole cost)
  auto family = [=](int which) -> int {
    for (int logn = 1; logn <= (which == 0 ? max_logn : max_logn_big); logn++) {
      const bool walk = logn <= 27;
      const int rc = which == 0 ? check(logn, 8, 32, true) : which == 1 ? check(logn, 8, 4, false, 36, false, walk) : check(logn, 8, 16, false, 8, true, walk);
      if (rc) return which * 1000000 + logn * 100 + rc;
    }
    return 0;
  };
  std::future<int> f1 = std::async(std::launch::async, family, 1), f2 = std::async(std::launch::async, family, 2);
  const int rc0 = family(0), rc1 = f1.get(), rc2 = f2.get();
  return rc0 ? rc0 : rc1 ? rc1 : rc2;
}

// the geometry big_ntt_run launches pass p of a 2^logn transform with: out = s, T, ntiles, tot, threads, LDS bytes; returns the pass count
extern "C" int big_pass_probe(int logn, int p, int elem_bytes, int tcap, int radix16, int* out)
{
  int parts[3], P;
  split_logn(logn, 8, parts, &P);
  if (p < 0 || p >= P) return -1;
  const BigPass bp = big_pass_geometry(parts, P, p, 1ull << logn, logn, (uint32_t)elem_bytes, (uint32_t)tcap, radix16 != 0);
  out[0] = bp.pd.s, out[1] = bp.pd.T, out[2] = (int)bp.pd.ntiles, out[3] = (int)bp.tot, out[4] = (int)bp.threads, out[5] = (int)bp.lds_bytes;
  return P;
}

// ---- lane-native launch geometry (ntt_plan.h fast_pass_geometry, the code ntt_run launches with) -----------------------------
// Grouping (cg adjacent logical columns in pass 0 / the last pass, ag adjacent outer indices in the middle pass) is a launch
// optimisation only: it must not change which word any logical element is read from or written to. For every pass, launch row
// (row group, slice, cs), tile, slot and live lane, the word address -- the kernels' formulas, k_ntt_fast LN -- is mapped back to
// (row group, element j, lane l) of that side's buffer and must be the one the ungrouped pass (cg_max = 1, same function) gives
// the same logical column / outer index; l < ltot (no padding lane), and the word lies inside the side's buffer.
namespace lanecheck {
  struct Side {
    uint64_t es, cst; // element stride, group stride (words)
  };
  static uint64_t brev(uint64_t x, uint32_t bits)
  {
    uint64_t r = 0;
    for (uint32_t i = 0; i < bits; i++)
      r |= ((x >> i) & 1ull) << (bits - 1 - i);
    return r;
  }
  // word of (launch row r, tile (a, ct) with a the kernel's first outer index, row k of the tile, logical column c of the
  // LDS tile, lane of the slice) on side `out`
  static uint64_t word(const FastPass& g, bool out, bool rn, uint32_t r, uint64_t a, uint64_t ct, uint64_t k, uint64_t c, uint32_t lane)
  {
    const PassDesc& pd = g.pd;
    const NttLaunch& nl = g.nl;
    const uint32_t cs = r % nl.cgrp, rs = r / nl.cgrp;
    const uint64_t es = out ? (nl.es_out ? nl.es_out : nl.es) : nl.es;
    const uint64_t roff = (uint64_t)(rs / nl.lanes) * nl.bs + ((uint64_t)(rs % nl.lanes) << nl.lsh) + (uint64_t)cs * (out ? nl.cst_out : nl.cst_in);
    const uint64_t in_base = a * pd.in_base_a + ct * pd.in_base_ct;
    uint64_t e;
    if (!out || !pd.is_last || rn) { // column passes on both sides, the row pass's load (in_sk = 1)
      e = in_base + k * pd.in_sk + c * pd.in_st;
    } else {
      const uint64_t K0 = (pd.pidx <= 1) ? (ct * pd.T + c) : (ct * pd.T + c + (uint64_t)pd.n0 * a);
      if (nl.out_rev) // bitrev(K0 + cs * tcl + k * out_sk) = bitrev_s(k) + L * bitrev(K0 + cs * tcl): tile row k holds bitrev_s(k)
        e = brev(K0 + (uint64_t)cs * nl.tcl, nl.logn - pd.s) * (1ull << pd.s) + k;
      else
        e = K0 + k * pd.out_sk;
    }
    return roff + e * es + lane;
  }

  struct Shape {
    uint32_t logn, batch, lanes;
    bool columns;
    int ord; // 0 kNN, 1 kNR, 2 kRN, 3 kRR
    bool coset, inverse;
  };

  static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
  static uint64_t rnd()
  {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
  }

  // 0 = every word right; else a code: 1 bad ungrouped plan, 2 lane out of range / padding lane, 3 outside the buffer,
  // 4 grouped word differs from the ungrouped one, 5 a word of the full map touched twice, 6 a live word never touched
  static int check_shape(const Shape& sh, bool sample)
  {
    int parts[3], P;
    ntt_split_parts((int)sh.logn, -1, parts, &P);
    const uint64_t n = 1ull << sh.logn;
    NttLaunch nl{};
    nl.logn = sh.logn, nl.n = n, nl.nbatch = sh.batch * sh.lanes, nl.lanes = sh.lanes;
    nl.bs = sh.columns ? sh.lanes : n * sh.lanes;
    nl.es = sh.columns ? (uint64_t)sh.batch * sh.lanes : sh.lanes;
    nl.in_rev = sh.ord == 2 || sh.ord == 3, nl.out_rev = sh.ord == 1 || sh.ord == 3;
    nl.inverse = sh.inverse, nl.coset = sh.coset, nl.log_max = 27;
    const NttPlanFlags f = ntt_plan_flags(P, nl.in_rev, nl.out_rev, nl.coset, nl.inverse, sh.columns, sh.batch, sh.lanes, nl.es, true, true, true);
    if (!f.lane_native) return 0;
    if (f.prerev) nl.in_rev = 0; // (ntt_run: the passes see natural-order rows in the work buffer)
    const uint32_t ltot = f.ltot;
    for (int p = 0; p < P; p++) {
      const bool src_w = !f.rn_native && (p > 0 || f.prerev), dst_w = !f.rn_native && p < P - 1; // (ntt_run's src / dst)
      const FastPassIn gi{parts, P, p, n, 27, f, sh.lanes, src_w, dst_w, true, 8u};
      FastPassIn ui = gi;
      ui.cg_max = 1;
      const FastPass G = fast_pass_geometry(nl, gi), U = fast_pass_geometry(nl, ui);
      if (U.cg != 1 || U.ag != 1 || U.tcl != G.tcl || U.lsh != G.lsh || (uint32_t)U.pd.T != U.tcl || U.nl.cgrp != 1) return 1;
      if (G.nl.cgrp != G.cg * G.ag || (uint32_t)G.pd.T != G.tcl * G.cg || (uint64_t)G.pd.ntiles * G.ag != U.pd.ntiles / G.cg) return 1;
      const uint64_t L = 1ull << parts[p];
      const uint32_t TL = 1u << G.lsh, slices = G.nl.lanes;
      if (slices != (ltot + TL - 1) / TL || G.nl.nrows_launch != f.row_groups * slices * G.nl.cgrp) return 1;
      for (int out = 0; out < 2; out++) {
        const uint64_t es = out ? (G.nl.es_out ? G.nl.es_out : G.nl.es) : G.nl.es;
        const uint64_t ues = out ? (U.nl.es_out ? U.nl.es_out : U.nl.es) : U.nl.es;
        if (es != ues || es < ltot) return 1;
        const uint64_t words = (uint64_t)f.row_groups * n * es;
        // full word map: every live word once. Sampled: the first and last tile of every outer index a (of 16 spread over the range
        // when there are more), plus 8 seeded tiles; the first and last slice and row group with every cs; in each tile the first
        // and last logical column, rows 0, L - 1 and a seeded one, the first and last live lane
        std::vector<uint8_t> seen;
        if (!sample) seen.assign(words, 0);
        std::vector<uint32_t> tiles, rows;
        const uint32_t na = G.pd.ntiles / G.pd.tiles_per_a;
        if (!sample) {
          for (uint32_t t = 0; t < G.pd.ntiles; t++)
            tiles.push_back(t);
          for (uint32_t r = 0; r < G.nl.nrows_launch; r++)
            rows.push_back(r);
        } else {
          const uint32_t nas = std::min<uint32_t>(na, 16);
          for (uint32_t i = 0; i < nas; i++) {
            const uint32_t ai = nas == 1 ? 0 : (uint32_t)((uint64_t)i * (na - 1) / (nas - 1));
            tiles.push_back(ai * G.pd.tiles_per_a);
            if (G.pd.tiles_per_a > 1) tiles.push_back(ai * G.pd.tiles_per_a + G.pd.tiles_per_a - 1);
          }
          for (int i = 0; i < 8; i++)
            tiles.push_back((uint32_t)(rnd() % G.pd.ntiles));
          for (uint32_t grp : {0u, f.row_groups - 1})
            for (uint32_t sl : {0u, slices - 1})
              for (uint32_t cs = 0; cs < G.nl.cgrp; cs++) {
                const uint32_t r = (grp * slices + sl) * G.nl.cgrp + cs;
                if (std::find(rows.begin(), rows.end(), r) == rows.end()) rows.push_back(r);
              }
        }
        for (uint32_t r : rows) {
          const uint32_t cs = r % G.nl.cgrp, rs = r / G.nl.cgrp, slice = rs % slices;
          const uint32_t live = std::min<uint32_t>(TL, ltot - slice * TL);
          for (uint32_t tile : tiles) {
            const uint64_t a = (uint64_t)(tile / G.pd.tiles_per_a) * G.ag, ct = tile % G.pd.tiles_per_a;
            // the same logical element in the ungrouped pass: column ct * T + cs * tcl + c (cg), outer index a + cs (ag)
            const uint64_t ua = G.ag > 1 ? a + cs : a;
            for (uint64_t c = 0; c < G.tcl; c += sample ? std::max<uint64_t>(1, G.tcl - 1) : 1) {
              const uint64_t col = ct * G.pd.T + (G.cg > 1 ? (uint64_t)cs * G.tcl : 0) + c;
              const uint64_t uct = col / U.tcl, uc = col % U.tcl;
              if (ua * U.pd.tiles_per_a + uct >= U.pd.ntiles || uct >= U.pd.tiles_per_a) return 1;
              const uint64_t ks[3] = {0, L - 1, rnd() % L};
              for (uint64_t ki = 0; ki < (sample ? 3 : L); ki++) {
                const uint64_t k = sample ? ks[ki] : ki;
                for (uint32_t lane = 0; lane < live; lane += sample ? std::max<uint32_t>(1, live - 1) : 1) {
                  const uint64_t w = word(G, out, f.rn_native, r, a, ct, k, c, lane);
                  if (w >= words) return 3;
                  const uint64_t grp = w / (n * es), j = (w % (n * es)) / es, l = w % es;
                  if (l >= ltot || l != (uint64_t)slice * TL + lane || grp != rs / slices) return 2;
                  const uint64_t wu = word(U, out, f.rn_native, rs, ua, uct, k, uc, lane);
                  if (wu != w || j >= n) return 4;
                  if (!sample && seen[w]++) return 5;
                }
              }
            }
          }
        }
        if (!sample) // every live word of the side once (the padding lanes never)
          for (uint64_t w = 0; w < words; w++)
            if ((w % es < ltot) != (seen[w] == 1)) return 6;
      }
    }
    return 0;
  }
} // namespace lanecheck

// Returns 0, or an encoded failing shape: code + 10 * (ord + 4 * (coset + 2 * inverse)) + 1000 * logn + 100000 * ltot
// (+ 50000000 for the extension field, + 100000000 for row-major). Sizes up to 2^14 words get the full word map (each live word
// exactly once), larger ones sampled tiles and rows of the tile.
extern "C" int lane_plan_check(int min_logn, int max_logn)
{
  using namespace lanecheck;
  std::vector<uint32_t> ltots;
  for (uint32_t t = 2; t <= 160; t++)
    ltots.push_back(t);
  ltots.push_back(192), ltots.push_back(256);
  for (uint32_t logn = (uint32_t)min_logn; logn <= (uint32_t)max_logn; logn++)
    for (int mode = 0; mode < 12; mode++) { // (without a coset the direction changes no address: forward only)
      const int ord = mode % 4;
      const bool coset = mode >= 4, inverse = mode >= 8;
      std::vector<Shape> shapes;
      for (uint32_t t : ltots) {
        shapes.push_back({logn, t, 1, true, ord, coset, inverse});                   // columns_batch, base field
        if (t % 4 == 0) shapes.push_back({logn, t / 4, 4, true, ord, coset, inverse}); // columns_batch, extension
      }
      for (uint32_t b : {1u, 2u, 3u})
        shapes.push_back({logn, b, 4, false, ord, coset, inverse}); // row-major extension rows: ltot = 4
      for (const Shape& sh : shapes) {
        const bool sample = (uint64_t)(1ull << logn) * sh.batch * sh.lanes > (1ull << 14);
        if (int rc = check_shape(sh, sample))
          return rc + 10 * (ord + 4 * ((int)coset + 2 * (int)inverse)) + 1000 * (int)logn + 100000 * (int)(sh.batch * (sh.columns ? sh.lanes : 1)) +
                 (sh.lanes == 4 ? 50000000 : 0) + (sh.columns ? 0 : 100000000);
      }
    }
  return 0;
}

// window groups of the pipelined MSM schedule: a partition of [0, tw) into contiguous non-empty ranges, highest first
extern "C" int msm_groups_check(void)
{
  for (int tw = 1; tw <= 200; tw++)
    for (int want = 1; want <= 20; want++) {
      int lo[MSM_MAX_GROUPS], hi[MSM_MAX_GROUPS];
      const int ng = msm_window_groups(tw, want, lo, hi);
      if (ng < 1 || ng > MSM_MAX_GROUPS || ng > std::max(1, want)) return 1000 * tw + want;
      if (tw < 4 && ng != 1) return -(1000 * tw + want);
      if (hi[0] != tw || lo[ng - 1] != 0) return 2000000 + 1000 * tw + want;
      for (int g = 0; g < ng; g++) {
        if (lo[g] >= hi[g]) return 3000000 + 1000 * tw + want;
        if (g + 1 < ng && lo[g] != hi[g + 1]) return 4000000 + 1000 * tw + want;
      }
    }
  return 0;
}

// shapes of a transform split over P device slots: both factors cover the slots, the factors multiply to N
extern "C" int split_shape_check(void)
{
  for (int logn = 0; logn <= 30; logn++)
    for (int P = 1; P <= 64; P++) {
      SplitShape s;
      const bool ok = split_shape(logn, P, &s);
      const bool pow2 = P >= 2 && (P & (P - 1)) == 0;
      int lp = 0;
      while ((1 << lp) < P)
        lp++;
      if (!pow2 && ok) return 100 * logn + P;
      if (ok && (s.a + s.b != logn || s.a < lp || s.b < lp || s.a < s.b)) return 10000 + 100 * logn + P;
      if (pow2 && !ok && logn >= 2 * lp) return 20000 + 100 * logn + P; // every transform with N >= P^2 can be split
    }
  return 0;
}

// the window plan msm() picks: window size inside the sort's range, never a top window of 1-3 scalar bits, batches of
// small MSMs on the one-level sort, a caller-set c honoured, precompute tables on a c that ignores batch_size
extern "C" int msm_plan_check(void)
{
  for (int bits : {254, 255, 64, 128})
    for (int logn = 0; logn <= 28; logn++)
      for (int batch : {1, 16, 1024})
        for (int pf : {1, 4}) {
          icicle_msm_config_t cfg{};
          cfg.batch_size = batch;
          cfg.precompute_factor = pf;
          const int n = 1 << logn;
          const MsmPlan p = make_plan(n, bits, cfg);
          const int tag = ((bits * 100 + logn) * 10 + (batch > 1)) * 10 + pf;
          if (p.c < 2 || p.c > (p.n_lo > 0 ? 22 : 21)) return tag * 10 + 1;
          if (p.n_lo > 0) { // mixed widths: they add up to the scalar bits, narrow windows below wide ones, full-width scalars only
            if (!p.negate || pf != 1 || batch != 1 || p.bits != bits || p.n_lo >= p.nwin) return tag * 10 + 2;
            if (p.offset(p.nwin - 1) + p.width(p.nwin - 1) != p.bits || p.nb != (1u << (p.c - 1)) || p.wpf != p.nwin) return tag * 10 + 2;
            if (logn < 23) return tag * 10 + 3; // never below 2^23 terms
            continue;
          }
          if (p.negate) return tag * 10 + 2;
          if (p.nwin != (p.bits + 1 + p.c - 1) / p.c || p.wpf != (p.nwin + pf - 1) / pf || p.nb != (1u << (p.c - 1))) return tag * 10 + 2;
          if (pf == 1 && p.nwin > 1 && p.bits > 8 && p.bits + 1 - p.c * (p.nwin - 1) <= 3) return tag * 10 + 3; // tiny top window
          if (pf == 1 && batch > 1 && logn <= 17 && p.c > 11) return tag * 10 + 4;
          // a single small MSM of full-width scalars: the latency rule (8 up to 2^12 terms, then 15 -- or the next c whose top window is no stub)
          if (pf == 1 && batch == 1 && logn < 18 && bits >= 200 && p.c != (logn <= 12 ? 8 : (bits == 255 ? 16 : 15))) return tag * 10 + 8;
          if (pf > 1) { // a base table: msm_precompute_bases and msm must agree whatever batch_size either call carries
            icicle_msm_config_t c1 = cfg;
            c1.batch_size = 1;
            if (make_plan(n, bits, c1).c != p.c) return tag * 10 + 5;
          }
          cfg.c = 13;
          if (make_plan(n, bits, cfg).c != 13) return tag * 10 + 6;
          if (p.seg < 64 || (p.seg & (p.seg - 1)) != 0) return tag * 10 + 7;
        }
  return 0;
}

// ECNTT stage plan + the index algebra of the radix-2^r matrix-form stages (ecntt.hip k_ecntt_terms / k_ecntt_sums), simulated
// over the integers mod a small prime with "points" = residues and "scalar multiplication" = modular product: a transform
// computed stage by stage with ecntt_term_exponent() must equal the O(n^2) definition for every width plan.
static uint64_t mpow(uint64_t b, uint64_t e, uint64_t p)
{
  uint64_t r = 1;
  b %= p;
  while (e) {
    if (e & 1) r = r * b % p;
    b = b * b % p;
    e >>= 1;
  }
  return r;
}
extern "C" int ecntt_plan_check(void)
{
  const uint64_t p = 7681; // 7681 - 1 = 2^9 * 15: roots of unity up to order 512
  const uint64_t g = 17;   // a primitive root mod 7681
  for (int logn = 0; logn <= 9; logn++)
    for (int forced = 0; forced <= 5; forced++)
      for (uint64_t budget : {(uint64_t)16384, (uint64_t)64}) {
        const uint64_t n = (uint64_t)1 << logn;
        int widths[64];
        const int nst = ecntt_stage_plan(logn, n, budget, forced, widths);
        int sum = 0;
        for (int i = 0; i < nst; i++) {
          if (widths[i] < 1 || widths[i] > 5 || (i && widths[i] > widths[i - 1])) return 1000 + logn * 10 + forced;
          if (forced == 0 && widths[i] > 1 && n * ((1ull << widths[i]) - 1) / 2 > budget) return 2000 + logn * 10;
          sum += widths[i];
        }
        if (sum != logn) return 3000 + logn * 10 + forced;
        if (logn == 0) continue;
        const uint64_t w = mpow(g, (p - 1) / n, p); // primitive n-th root
        std::vector<uint64_t> x(n), work(n), next(n);
        for (uint64_t i = 0; i < n; i++)
          x[i] = (i * i * 31 + 7 * i + 3) % p;
        for (uint64_t i = 0; i < n; i++) { // DIT input: bit-reversed
          uint64_t j = 0;
          for (int b = 0; b < logn; b++)
            j |= ((i >> b) & 1) << (logn - 1 - b);
          work[i] = x[j];
        }
        int q0 = 0;
        for (int si = 0; si < nst; si++) {
          const int r = widths[si];
          const uint64_t R = 1ull << r, hr = R >> 1, L = 1ull << q0, M = L * R;
          const uint64_t wM = mpow(w, n / M, p);
          for (uint64_t g0 = 0; g0 < n / R; g0++) {
            const uint64_t pos = g0 & (L - 1), blk = g0 >> q0, base = (blk << (q0 + r)) + pos;
            for (uint64_t u = 0; u < hr; u++) {
              uint64_t ev = work[base], od = 0;
              for (uint64_t j = 1; j < R; j++) {
                const uint64_t t = work[base + j * L] * mpow(wM, ecntt_term_exponent(q0, r, (uint32_t)j, (uint32_t)u, pos), p) % p;
                if (j < hr)
                  ev = (ev + t) % p;
                else
                  od = (od + t) % p;
              }
              next[base + u * L] = (ev + od) % p;
              next[base + (u + hr) * L] = (ev + p - od) % p;
            }
          }
          work.swap(next);
          q0 += r;
        }
        for (uint64_t k = 0; k < n; k++) {
          uint64_t acc = 0;
          for (uint64_t j = 0; j < n; j++)
            acc = (acc + x[j] * mpow(w, j * k % n, p)) % p;
          if (acc != work[k]) return 4000 + logn * 10 + forced;
        }
      }
  return 0;
}

// ECNTT route (ntt_plan.h ecntt_route, what ecntt_run launches) for one shape and one set of overrides: out[0] = stages, out[1] = rmax,
// out[2] = stage_gtab, out[3] = scale pass runs, out[4] = scale_gtab, out[5] = budget, out[6 + i] = width of stage i. logn and tot are
// separate arguments so that a test can put tot on either side of a boundary whatever the transform size (the function reads tot only).
extern "C" int ecntt_route_probe(int point_bytes, int logn, uint64_t tot, int inverse, int coset, int forced_r, uint64_t budget, int gtab_mode, int* out)
{
  EcnttOverrides ov;
  ov.forced_r = forced_r, ov.budget = budget, ov.gtab_mode = gtab_mode;
  const EcnttRoute rt = ecntt_route((size_t)point_bytes, logn, tot, inverse != 0, coset != 0, ov);
  out[0] = rt.nst, out[1] = rt.rmax, out[2] = rt.stage_gtab, out[3] = rt.scale_runs, out[4] = rt.scale_gtab, out[5] = (int)rt.budget;
  for (int i = 0; i < rt.nst; i++)
    out[6 + i] = rt.widths[i];
  return 0;
}

// ---- MSM launch decisions (msm_plan.h), each for one shape and one set of knobs. knobs[]: hb_set, hb, mrow_set, mrow, acc_waves_set,
// acc_waves, reduce_balance, reduce_small, reduce_quad, host_combine, batch_horner (tests/test_plan.py _knobs) ----
static MsmKnobs probe_knobs(const int* k)
{
  MsmKnobs kn;
  kn.hb_set = k[0] != 0, kn.hb = k[1], kn.mrow_set = k[2] != 0, kn.mrow = k[3], kn.acc_waves_set = k[4] != 0, kn.acc_waves = k[5];
  kn.reduce_balance = k[6] != 0, kn.reduce_small = k[7] != 0, kn.reduce_quad = k[8] != 0, kn.host_combine = k[9] != 0, kn.batch_horner = k[10] != 0;
  return kn;
}
// returns whether the shape fits the sort; out = hb, lb, jb, chunk_log, nblk
extern "C" int msm_sort_probe(int n, int c, int pf, const int* knobs, int* out)
{
  SortPlan sp{};
  if (!msm_sort_plan(n, c, pf, probe_knobs(knobs), &sp)) return 0;
  out[0] = sp.hb, out[1] = sp.lb, out[2] = sp.jb, out[3] = sp.chunk_log, out[4] = sp.nblk;
  return 1;
}
// geometry of (batch, wpf, nb, rwl), then the route of windows [w0, w0 + nw) on it; seg_lo / nsegr < 0: the whole window.
// out = mrow, m, nseg, log_chunk | chunk kernel (0 none, 1 wave_quad, 2 small, 3 wave), window kernel (0 none, 1 window_quad,
// 2 window), direct, nlo_w, nsq, mq, lw_log, per_wave, nblocks, mrow_lo, nseg_lo, log_chunk_lo, wchunks, wchunk_size, wthreads, cost_q, cost_s
extern "C" int msm_reduce_probe(int batch, int wpf, uint32_t nb, uint32_t rwl, int w0, int nw, int n_lo, int seg_lo, int nsegr, int has_hook, int NG, int bb, int quad_ok,
                                const int* knobs, int* out)
{
  const MsmKnobs kn = probe_knobs(knobs);
  const MsmReduceGeom g = msm_reduce_geom(batch, wpf, nb, rwl, kn);
  out[0] = (int)g.mrow, out[1] = (int)g.m, out[2] = (int)g.nseg, out[3] = (int)g.log_chunk;
  const MsmReduceRoute r = msm_reduce_route(nb, w0, nw, n_lo, g, seg_lo < 0 ? 0u : (uint32_t)seg_lo, nsegr < 0 ? g.nseg : (uint32_t)nsegr, has_hook != 0, NG, bb, quad_ok != 0, rwl, kn);
  out[4] = (int)r.chunk, out[5] = (int)r.window, out[6] = r.direct, out[7] = (int)r.nlo_w, out[8] = (int)r.nsq, out[9] = (int)r.mq, out[10] = (int)r.lw_log;
  out[11] = (int)r.per_wave, out[12] = (int)r.nblocks, out[13] = (int)r.mrow_lo, out[14] = (int)r.nseg_lo, out[15] = (int)r.log_chunk_lo;
  out[16] = (int)r.wchunks, out[17] = (int)r.wchunk_size, out[18] = (int)r.wthreads, out[19] = (int)r.cost_q, out[20] = (int)r.cost_s;
  return 0;
}
// 0 host, 1 k_final_horner, 2 k_final, 3 k_final + k_final_combine
extern "C" int msm_combine_probe(int results_on_device, int is_async, int batch, int bb, int has_hook, int wpf, const int* knobs)
{
  return (int)msm_combine_route(results_on_device != 0, is_async != 0, batch, bb, has_hook != 0, wpf, probe_knobs(knobs));
}
// out = MINW, PAD of the k_accumulate instantiation
extern "C" int msm_acc_probe(int is_g2, int xyzz_bytes, int limbs, int co_ok, const int* knobs, int* out)
{
  const MsmAccWaves aw = msm_acc_waves(is_g2 != 0, (size_t)xyzz_bytes, limbs, co_ok != 0, probe_knobs(knobs));
  out[0] = aw.minw, out[1] = aw.pad;
  return 0;
}
// BB of msm_batch_fold for a plan made by make_plan (0: a hook's batch does not fit one launch group)
extern "C" int msm_fold_probe(int n, int bits, int batch, int c, int proj_bytes, uint64_t staged_base_bytes, uint64_t free_bytes, int has_hook, const int* knobs)
{
  icicle_msm_config_t cfg{};
  cfg.batch_size = batch, cfg.c = c;
  const MsmPlan pl = make_plan(n, bits, cfg);
  SortPlan sp{};
  if (!msm_sort_plan(n, pl.c, pl.pf, probe_knobs(knobs), &sp)) return -1;
  return msm_batch_fold(pl, sp, n, (size_t)proj_bytes, (size_t)staged_base_bytes, (size_t)free_bytes, batch, has_hook != 0);
}
// the window plan msm() makes for one MSM of n terms with config.c = c (0: the cost model): out = c, nwin, wpf, nb, n_lo
extern "C" int msm_plan_probe(int n, int bits, int c, int* out)
{
  icicle_msm_config_t cfg{};
  cfg.batch_size = 1, cfg.c = c;
  const MsmPlan pl = make_plan(n, bits, cfg);
  out[0] = pl.c, out[1] = pl.nwin, out[2] = pl.wpf, out[3] = (int)pl.nb, out[4] = pl.n_lo;
  return 0;
}
// the whole plan of one launch sequence, as msm() makes it: out = c, nwin, wpf, nb, n_lo, negate, seg. batch, pf, bitsize: MSMConfig's
// batch_size, precompute_factor, bitsize; force_windows: MSMConfig.ext "hip_msm_windows"
extern "C" int msm_plan_seg_probe(int n, int bits, int c, int batch, int pf, int bitsize, int force_windows, int* out)
{
  icicle_msm_config_t cfg{};
  cfg.batch_size = batch, cfg.c = c, cfg.precompute_factor = pf, cfg.bitsize = bitsize;
  const MsmPlan pl = make_plan(n, bits, cfg, force_windows);
  out[0] = pl.c, out[1] = pl.nwin, out[2] = pl.wpf, out[3] = (int)pl.nb, out[4] = pl.n_lo, out[5] = pl.negate ? 1 : 0, out[6] = (int)pl.seg;
  return 0;
}
