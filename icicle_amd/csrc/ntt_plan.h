// Pass decomposition shared by the 31-bit NTT (ntt.hip) and the 256-bit scalar-field NTT (ntt_big.hip).
//
// N = N0*N1[*N2] is split into at most three passes; pass p computes 2^s-point sub-transforms on
// [L x T] tiles (T adjacent columns => every HBM access is a run of T contiguous elements), applies
// the inter-pass twiddle on the way out, and the LAST pass scatters straight into natural order.
// Addresses are in ELEMENTS of one logical row; the kernels scale by the element stride / width.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace icicle_hip {

  // ---- pass descriptor -------------------------------------------------------------------------
  struct PassDesc {
    int s;            // log2 of the sub-transform length L
    int T;            // tile width (columns per block)
    uint32_t ntiles;  // tiles per row-transform
    // tile -> (a, c0): tile index = a * tiles_per_a + ct ;
    uint32_t tiles_per_a;
    // load/store addressing inside one logical row: addr = base + k*sk + t*st
    uint64_t in_base_a, in_base_ct, in_sk, in_st;     // base = a*in_base_a + ct*in_base_ct
    uint64_t out_sk, out_st;                          // out base computed in-kernel (needs digit reversal)
    int is_last;      // last pass: natural-order scatter + optional 1/N scaling
    int pidx;         // pass index
    int xcd_remap;    // fast path: blockIdx.x -> tile map that keeps neighbouring tiles on one XCD
    // twiddle after this pass (not last): exponent = jnext * K, table stride tstride
    uint64_t tw_stride;  // max / M
    uint32_t cprime;     // C' = C / N_{p+1}; jnext = (c0 + t) / C'
    uint32_t n0, n1;     // N_0, N_1 (for K and digit reversal)
    // bit-reversed INPUT consumed natively (kRN, ntt_fast.hpp RN != 0): in-place DIT by digits. Pass q transforms digit j_q
    // (rows in bit-reversed order in memory, read as they lie) into k_q (rows in natural order); the columns of pass q >= 1 are
    // the A_q = N_0 .. N_{q-1} low output digits already produced, the outer index `a` is the bit reversal of the digits still
    // to come. rn_first: pass 0, whose rows are the elements of a contiguous run (the tile's columns are runs, not output digits).
    // rn_next_bits = log2 N_{q+1}: the factor behind pass q is w_{M}^(j_{q+1} * (column + A_q * row)), j_{q+1} = bitrev(a mod N_{q+1}).
    int rn_first = 0, rn_next_bits = 0;
  };

  struct NttLaunch {
    uint32_t logn;
    uint64_t n;
    uint32_t nbatch;   // number of independent lane-transforms (batch * lanes)
    uint32_t lanes;    // 1 (scalar) or 4 (quartic extension)
    uint64_t bs;       // offset(b') = (b'/lanes)*bs + (b'%lanes)
    uint64_t es;       // element stride (of the pass's source)
    // element stride of the pass's DESTINATION when it differs (0 = es). Interleaved transforms whose count is not a multiple of
    // 32 (columns_batch with 100 columns: rows of 400 bytes) make every 128-byte access of every pass straddle three 64-byte sectors
    // instead of two (2.9 TB/s per pass against 4.8, profiles/r05_notes.md section 5). Only the passes that touch the CALLER's
    // buffers have to see that layout: the work buffer between the passes pads the lane count to a multiple of 32 words, so of the
    // six memory sides of a three-pass transform four are sector-aligned (the padding lanes are never read or written).
    uint64_t es_out = 0;
    int in_rev, out_rev; // bit-reversed logical->memory maps
    int inverse;
    uint32_t log_max;
    uint32_t ninv_mont;  // N^-1 (Montgomery) for inverse
    int coset;           // multiply by powers table (forward: on first load; inverse: on last store)
    // row-group execution (fast path): this launch covers rows [row0, row0 + nrows_launch); a buffer
    // flagged "relative" holds only the current group (its row r lives at offset of row r - row0)
    uint32_t row0 = 0, nrows_launch = 0;
    int src_rel = 0, dst_rel = 0;
    // lane-native tiles (ntt_fast.hpp, LN): `ltot` transforms interleaved word by word, a launch row = one slice of
    // 2^lsh of them; `lanes` then counts the slices per row group: offset(r) = (r / lanes) * bs + ((r % lanes) << lsh)
    uint32_t lsh = 0, ltot = 1;
    // lane-native, few slices (16-64 interleaved transforms): `cgrp` ADJACENT logical columns share one twiddle set in pass 0
    // (same w_M^(jnext K): jnext = column / cprime) and in the last pass (no inter-pass factor at all), so they run as launch
    // rows of one block: row r = (row group, slice, column cs), cs = r % cgrp, at word offsets cs * cst_in / cs * cst_out
    // In the middle pass of a three-pass transform the factor is w^(column * (a + n0 k)): there `agrp` adjacent values of the OUTER
    // index a run as the rows of a block (agrp = cgrp), w^(column * a) being applied per row to the loaded operands.
    uint32_t cgrp = 1, agrp = 1;
    int vec4 = 0;     // RN run pass: unit element stride and 16-byte aligned rows -- a thread's 16 consecutive words load as 4 x uint4
    uint32_t tcl = 1; // logical columns in the LDS tile (PassDesc::T counts the cgrp-wide group in pass 0 / the last pass)
    uint64_t cst_in = 0, cst_out = 0;
  };

#if defined(__HIPCC__)
  __device__ __forceinline__ uint64_t bitrev64(uint64_t x, uint32_t bits)
  {
    return bits == 0 ? 0 : (__brevll(x) >> (64 - bits));
  }
#endif


  // <= 3 passes; sub-transforms of at most 2^smax points while that covers logn, larger above
  static inline void split_logn(int logn, int smax, int* parts, int* np)
  {
    const int SMAX = std::max(smax, (logn + 2) / 3);
    const int P = std::max(1, (logn + SMAX - 1) / SMAX);
    for (int i = 0; i < P; i++)
      parts[i] = logn / P + (i < logn % P ? 1 : 0);
    *np = P;
  }

  // descriptor of pass p of P; tmax = widest tile the kernel's LDS / block budget allows for 2^parts[p] rows
  static inline PassDesc make_pass(const int* parts, int P, int p, uint64_t n, int log_max, uint32_t tmax)
  {
    PassDesc pd{};
    pd.s = parts[p];
    pd.pidx = p;
    pd.is_last = (p == P - 1);
    const uint64_t L = (uint64_t)1 << pd.s;
    uint64_t A = 1, C = 1;
    for (int q = 0; q < p; q++)
      A <<= parts[q];
    for (int q = p + 1; q < P; q++)
      C <<= parts[q];
    pd.n0 = 1u << parts[0];
    pd.n1 = P > 1 ? (1u << parts[1]) : 1;
    if (!pd.is_last) {
      pd.T = (int)std::min<uint64_t>(tmax, C);
      pd.tiles_per_a = (uint32_t)(C / pd.T);
      pd.ntiles = (uint32_t)(A * pd.tiles_per_a);
      pd.in_base_a = L * C;
      pd.in_base_ct = pd.T;
      pd.in_sk = C;
      pd.in_st = 1;
      int lm = 0; // M = N_0..N_{p+1}
      for (int q = 0; q <= p + 1; q++)
        lm += parts[q];
      pd.tw_stride = (uint64_t)1 << (log_max - lm);
      pd.cprime = (uint32_t)(C >> parts[p + 1]);
    } else {
      // tile over k0 (the slowest digit of a); for P==3 `a` in the kernel carries k1
      const uint64_t n0 = P >= 2 ? ((uint64_t)1 << parts[0]) : 1;
      const uint64_t n1 = P == 3 ? ((uint64_t)1 << parts[1]) : 1;
      pd.T = (int)std::min<uint64_t>(tmax, n0);
      pd.tiles_per_a = (uint32_t)(n0 / pd.T);
      pd.ntiles = (uint32_t)(n1 * pd.tiles_per_a);
      // row index = k0*n1 + k1 ; row start = row*L
      pd.in_base_a = L; // a = k1
      pd.in_base_ct = (uint64_t)pd.T * n1 * L;
      pd.in_sk = 1;
      pd.in_st = n1 * L;
      pd.out_sk = n >> pd.s;
      pd.out_st = 1;
    }
    return pd;
  }

  // Pass q of the native bit-reversed-input pipeline (see PassDesc::rn_first). run_pass: pass 0 of a row-major batch, run by
  // the RN == 2 code (lanes along the run); otherwise pass 0 has the column shape too (lane-native tiles: the tile's word-columns
  // are interleaved transforms, a row = one position of the run).
  static inline PassDesc make_pass_rn(const int* parts, int P, int q, int log_max, uint32_t tmax)
  {
    PassDesc pd{};
    pd.s = parts[q];
    pd.pidx = q;
    pd.is_last = (q == P - 1);
    const uint64_t L = (uint64_t)1 << pd.s;
    uint64_t C = 1, O = 1; // columns = low output digits done; outer = input digits still to come
    for (int i = 0; i < q; i++)
      C <<= parts[i];
    for (int i = q + 1; i < P; i++)
      O <<= parts[i];
    pd.n0 = 1u << parts[0];
    pd.n1 = P > 1 ? (1u << parts[1]) : 1;
    pd.rn_first = (q == 0);
    if (q == 0) { // tile = T runs of L contiguous elements
      pd.T = (int)std::min<uint64_t>(tmax, O);
      pd.tiles_per_a = (uint32_t)(O / pd.T);
      pd.ntiles = pd.tiles_per_a;
      pd.in_base_a = 0;
      pd.in_base_ct = (uint64_t)pd.T * L;
      pd.in_sk = 1;
      pd.in_st = L;
    } else {
      pd.T = (int)std::min<uint64_t>(tmax, C);
      pd.tiles_per_a = (uint32_t)(C / pd.T);
      pd.ntiles = (uint32_t)(O * pd.tiles_per_a);
      pd.in_base_a = L * C;
      pd.in_base_ct = pd.T;
      pd.in_sk = C;
      pd.in_st = 1;
    }
    if (!pd.is_last) {
      int lm = 0; // M = N_0 .. N_{q+1}
      for (int i = 0; i <= q + 1; i++)
        lm += parts[i];
      pd.tw_stride = (uint64_t)1 << (log_max - lm);
      pd.rn_next_bits = parts[q + 1];
    }
    return pd;
  }

  // ---- launch geometry of one pass of the 256-bit / Goldilocks NTT (ntt_big.hip big_ntt_run), host-callable so that
  // tests/plan_harness.cpp checks the very same code. elem_bytes: an element in LDS (36 B: 9 limbs of a 256-bit field, 8 B: goldilocks);
  // tcap: the widest tile (runs of >= 128 B in HBM: 4 elements of 32 B, 16 of 8 B); radix16: goldilocks' four stages per LDS trip.
  struct BigPass {
    PassDesc pd;
    uint32_t tmax;      // widest tile the LDS budget allows for 2^parts[p] rows
    uint32_t tot;       // elements of a tile, L * pd.T
    uint32_t threads;   // blockDim.x
    uint64_t lds_bytes; // dynamic LDS of the launch
  };
  static inline BigPass big_pass_geometry(const int* parts, int P, int p, uint64_t n, int log_max, uint32_t elem_bytes, uint32_t tcap, bool radix16)
  {
    BigPass bp{};
    const uint64_t L = (uint64_t)1 << parts[p];
    // tile of L x T elements, <= 72 KiB so that two blocks share a CU
    uint32_t tmax = tcap;
    while (tmax > 1 && L * tmax * elem_bytes > 72 * 1024)
      tmax >>= 1;
    bp.tmax = tmax;
    bp.pd = make_pass(parts, P, p, n, log_max, tmax);
    bp.tot = (uint32_t)(L * bp.pd.T);
    // one thread per 4-element group of a stage pair; goldilocks: per 16-element group of four stages (when the pass has four)
    bp.threads = std::max(64u, std::min(512u, bp.tot / ((radix16 && parts[p] >= 4) ? 16u : 4u)));
    bp.lds_bytes = (uint64_t)bp.tot * elem_bytes;
    return bp;
  }

  // ---- the 31-bit NTT's plan (ntt.hip ntt_run), host-callable so that tests/plan_harness.cpp checks the very same code ----------
  // Pass lengths: split_logn, then which pass takes the extra bit of a size that is not a multiple of three (`order` =
  // ICICLE_HIP_NTT_PARTS_ORDER, -1 = default). Measured (profiles/r05_ntt_big_parts.txt, 0 / 1 / 2 = first / last / middle): at 2^25
  // the MIDDLE pass is the place for the 512-row sub-transform, 8,9,8: 6.48 -> 6.02 ms (x 32 rows); every other size measured
  // (2^20, 2^22, 2^26, 2^27) is best or within 3 % with the default, so only 2^25 changes.
  static inline void ntt_split_parts(int logn, int order, int* parts, int* np)
  {
    // sub-transforms of 2^8 points (three passes at 2^24). Two passes of 2^12 (1024-thread blocks, 4-column tiles)
    // and 64-column tiles were built and measured in round 1 and lost: profiles/r01_notes.md.
    split_logn(logn, 8, parts, np);
    if (*np == 3 && order == 1) std::swap(parts[0], parts[2]);
    if (*np == 3 && (order == 2 || (order < 0 && logn == 25))) {
      std::swap(parts[0], parts[1]);
      if (parts[0] > parts[2]) std::swap(parts[0], parts[2]);
    }
  }

  // Transform-level choices: which kernel family runs the passes and how interleaved transforms are laid out in the work buffer.
  struct NttPlanFlags {
    bool rn_native;   // kRN consumed natively (ntt_fast.hpp RN): every pass in place in the output, no work buffer
    bool prerev;      // bit-reversed input reordered into the work buffer first (kRR, forward cosets on reversed input)
    bool fast;        // k_ntt_fast passes (else the generic kernel: single-pass transforms with reversed input)
    bool lane_native; // interleaved transforms (columns_batch, extension field) on lane-native tiles
    bool pad_w;       // the work buffer pads the lane count to a multiple of 32 words (NttLaunch::es_out)
    uint32_t ltot;    // interleaved transforms per row group
    uint32_t row_groups;
    uint64_t es_w;    // element stride in the work buffer
  };
  // es: the caller's element stride; *_on: the A/B switches ICICLE_HIP_NTT_RN_NATIVE / _LANES / _PAD_LANES. (The experimental row
  // groups of ntt_run, ICICLE_HIP_NTT_GROUP_MB, take row-major base-field batches only: never a padded work buffer.)
  static inline NttPlanFlags ntt_plan_flags(int P, bool in_rev, bool out_rev, bool coset, bool inverse, bool columns_batch, uint32_t batch, uint32_t lanes,
                                            uint64_t es, bool rn_on, bool lanes_on, bool pad_on)
  {
    NttPlanFlags f{};
    f.rn_native = rn_on && in_rev && !out_rev && !(coset && !inverse);
    f.prerev = in_rev && P >= 2 && !f.rn_native;
    f.fast = !in_rev || f.prerev || f.rn_native;
    // (A ragged lane count -- 100 columns -- is NOT slow because of its masked last slice: with the 4 surplus lanes split off into a
    //  row-major side batch the three full slices took as long as the four did, 0.85 vs 0.84 ms at 2^20 x 100. Rows of 100 words are
    //  400 bytes apart, so every 128-byte access straddles three 64-byte sectors instead of two: 2.9 TB/s per pass against 4.8 for the
    //  row batch. Built, measured, removed: profiles/r05_notes.md.)
    f.ltot = columns_batch ? batch * lanes : lanes;
    f.lane_native = lanes_on && f.fast && f.ltot > 1;
    f.row_groups = columns_batch ? 1u : batch;
    // Ragged interleaved layouts (columns_batch with a lane count that is not a multiple of 32 words: the Rust suite's 100
    // columns): the WORK buffer pads the lane count to the next multiple of 32, so that only the two passes that touch the
    // caller's buffers see rows that straddle sectors (NttLaunch::es_out).
    f.pad_w = pad_on && f.lane_native && columns_batch && P >= 2 && !f.prerev && !f.rn_native && f.ltot > 32 && f.ltot % 32 != 0;
    f.es_w = f.pad_w ? (uint64_t)((f.ltot + 31) / 32) * 32 : es;
    return f;
  }

  // One pass of the fast path: what ntt_run launches for pass p.
  struct FastPassIn {
    const int* parts;
    int P, p;
    uint64_t n;
    int log_max;
    NttPlanFlags f;
    uint32_t lanes;     // u32 words per element: 1, or 4 (quartic extension)
    bool src_w, dst_w;  // the pass reads / writes the work buffer
    bool big_on;        // ICICLE_HIP_NTT_BIG
    uint32_t cg_max;    // ICICLE_HIP_NTT_COLUMN_GROUP (8); 1 = no column / outer-index groups
  };
  struct FastPass {
    PassDesc pd;     // grouped descriptor (pd.T = tcl * cg logical columns, pd.ntiles counts groups of ag outer indices)
    NttLaunch nl;    // the launch's NttLaunch (strides of both sides, lane-native rows, group strides)
    uint32_t tmax;   // widest tile the LDS / block budget allows, in word-columns
    uint32_t lsh;    // lane-native: log2 of the interleaved transforms per launch row (slice)
    uint32_t tcl;    // logical columns in the LDS tile
    uint32_t cg, ag; // column groups (pass 0 / last pass), outer-index groups (middle pass)
    bool big;        // 1024-thread blocks (transforms of 2^27 points and more)
    int rn_mode;     // 0: not RN, 1: RN column pass, 2: RN run pass (pass 0 of a row-major batch)
  };
  static inline FastPass fast_pass_geometry(const NttLaunch& nl, const FastPassIn& in)
  {
    FastPass fp{};
    const NttPlanFlags& f = in.f;
    const int* parts = in.parts;
    const int P = in.P, p = in.p;
    const uint64_t L = (uint64_t)1 << parts[p];
    // block = T * L/16 threads (<= 512), LDS = 2 buffers of L*(T+1) words (<= 160 KiB)
    const uint64_t epb = L >= 16 ? 16 : L;
    const bool cvar = nl.coset && (nl.inverse ? p == P - 1 : p == 0); // coset factors in this pass
    // column passes of 512 / 1024 rows (transforms of 2^25 points and more): 1024-thread blocks, twice the tile width.
    // Measured (profiles/r03_notes.md section 9): 2^27 x 4 5.63 -> 5.18 ms, 2^27 x 8 9.74 -> 9.15, but 2^26 x 16 7.25 -> 7.52 and
    // 2^25 x 32 unchanged (one 16-wave block per CU hides less latency than two 8-wave ones): only from 2^27 up.
    fp.big = in.big_on && f.fast && !f.rn_native && !f.lane_native && nl.logn >= 27 && p < P - 1 && P >= 2 && (parts[p] == 9 || parts[p] == 10) && !cvar;
    uint32_t tmax = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(32, (fp.big ? 1024 : 512) * epb / L));
    while (tmax > 1 && 2 * L * (tmax + 1) * 4 > 160 * 1024)
      tmax >>= 1;
    fp.rn_mode = !f.rn_native ? 0 : ((p == 0 && !f.lane_native) ? 2 : 1);
    while (fp.rn_mode == 2 && tmax > 1 && 2 * (L + (L >> 4)) * tmax * 4 > 160 * 1024)
      tmax >>= 1;
    fp.tmax = tmax;
    // lane-native: the tile's tmax word-columns are (tmax >> lsh) logical columns x 2^lsh interleaved transforms. A lane count
    // that is not a multiple of the widest slice keeps a masked last slice (running the remainder as a second launch on
    // narrower slices -- 100 columns = 3 x 32 + a launch of 4-lane tiles -- was built and measured SLOWER, 2^20 x 100:
    // 0.79 -> 0.99 ms: the tail's logical columns are es * 4 bytes apart, 16-byte runs; profiles/r04_notes.md section 1).
    uint32_t lsh = 0;
    if (f.lane_native)
      while ((2u << lsh) <= tmax && (1u << lsh) < f.ltot)
        lsh++;
    fp.lsh = lsh;
    PassDesc pd = f.rn_native ? make_pass_rn(parts, P, p, in.log_max, tmax >> lsh) : make_pass(parts, P, p, in.n, in.log_max, tmax >> lsh);
    // Few launch rows (16-64 interleaved transforms = one or two slices): adjacent logical columns that share a twiddle set
    // run as launch rows of one block -- pass 0 (its inter-pass factor depends on column / cprime only) and the last pass
    // (none at all); not the coset / bit-reversed-output variants, whose per-block constants depend on the column.
    uint32_t cg = 1, ag = 1;
    const uint32_t tcl = (uint32_t)pd.T; // logical columns in the LDS tile
    {
      // (only with full slices: grouping multiplies the mostly idle rows of a ragged last slice as well -- 2^20 x 100: 0.84 -> 0.89 ms)
      const bool full = f.lane_native && f.fast && f.ltot % (1u << lsh) == 0;
      // (RN: every pass can group adjacent logical columns -- the factor behind a pass is rebuilt per row, ntt_fast.hpp rn_rowfac)
      const bool allowed = full && !cvar && (f.rn_native ? P >= 2 : ((p == 0 && P >= 2) || p == P - 1)); // (round 5: the bit-reversed-output store too)
      const bool middle = full && !f.rn_native && P == 3 && p == 1; // groups over the outer index instead (NttLaunch::agrp)
      const uint32_t rows_now = f.row_groups * ((f.ltot + (1u << lsh) - 1) >> lsh);
      uint32_t want = 1;
      while ((allowed || middle) && want * 2 <= in.cg_max && rows_now * want * 2 <= 8)
        want *= 2;
      if (middle) {
        while (want > 1 && ((uint64_t)1 << parts[0]) % want != 0)
          want >>= 1;
        ag = want;
        want = 1;
        pd.ntiles /= ag; // tiles enumerate (a / ag, ct)
      }
      while (want > 1) {
        const PassDesc pg = f.rn_native ? make_pass_rn(parts, P, p, in.log_max, tcl * want) : make_pass(parts, P, p, in.n, in.log_max, tcl * want);
        if ((uint32_t)pg.T == tcl * want && (f.rn_native || pg.is_last || (uint32_t)pg.T <= pg.cprime)) {
          pd = pg;
          cg = want;
          break;
        }
        want >>= 1;
      }
    }
    fp.tcl = tcl, fp.cg = cg, fp.ag = ag;
    NttLaunch nlp = nl;
    if (f.pad_w) { // the work buffer's rows are es_w words apart, the caller's ltot
      nlp.es = in.src_w ? f.es_w : nl.es;
      nlp.es_out = in.dst_w ? f.es_w : nl.es;
    }
    if (f.lane_native) { // launch rows = slices of 2^lsh transforms
      nlp.lsh = lsh;
      nlp.ltot = f.ltot;
      nlp.lanes = (f.ltot + (1u << lsh) - 1) >> lsh;
      nlp.bs = in.n * in.lanes;
      nlp.row0 = 0;
      nlp.tcl = tcl;
      nlp.cgrp = cg * ag;
      nlp.agrp = ag;
      const uint64_t es_in = nlp.es, es_out = nlp.es_out ? nlp.es_out : nlp.es; // (pad_w: each side with its own stride)
      nlp.cst_in = ag > 1 ? pd.in_base_a * es_in : (uint64_t)tcl * pd.in_st * es_in;
      if (f.rn_native) // (RN passes are in place: same layout both sides)
        nlp.cst_out = nlp.cst_in;
      else if (pd.is_last && nl.out_rev) // (the bit-reversed store computes the column's place itself, ntt_fast.hpp)
        nlp.cst_out = 0;
      else if (pd.is_last && ag == 1)
        nlp.cst_out = (uint64_t)tcl * es_out;
      else
        nlp.cst_out = ag > 1 ? pd.in_base_a * es_out : (uint64_t)tcl * pd.in_st * es_out;
      nlp.nrows_launch = f.row_groups * nlp.lanes * nlp.cgrp;
    }
    fp.pd = pd;
    fp.nl = nlp;
    return fp;
  }

  // ---- one transform split over P device slots (ntt_split.hpp): N = 2^a * 2^b, both factors at least P wide ----
  struct SplitShape {
    int P, logn, a, b; // N1 = 2^a, N2 = 2^b
  };
  static inline bool split_shape(int logn, int P, SplitShape* s, bool allow_one = false)
  { // (P = 1: the "hip_force_rccl" rehearsal of the exchanges on a single device slot)
    if (P < (allow_one ? 1 : 2) || (P & (P - 1)) != 0) return false;
    int lp = 0;
    while ((1 << lp) < P)
      lp++;
    const int a = std::max((logn + 1) / 2, lp), b = logn - a;
    if (b < lp || (P == 1 && b < 1)) return false;
    *s = {P, logn, a, b};
    return true;
  }

  // ---- ECNTT stage plan (ecntt.hip): radix-2^r "matrix form" stages ---------------------------------------------------
  // r = the largest value <= 5 whose tot (2^r - 1) / 2 scalar multiplications per stage stay within `budget` quads (one round
  // of quads on the chip); forced_r > 0 overrides. widths[] receives the stage widths (as even as possible, sum = logn),
  // returns their count; r = 1 everywhere means the plain radix-2 kernel.
  static inline int ecntt_stage_plan(int logn, uint64_t tot, uint64_t budget, int forced_r, int* widths)
  {
    int rmax = 1;
    if (forced_r > 0) {
      rmax = std::min(5, forced_r);
    } else {
      while (rmax < 5 && tot * ((2ull << rmax) - 1) / 2 <= budget)
        rmax++;
    }
    rmax = std::max(1, std::min(rmax, std::max(1, logn)));
    const int nst = logn > 0 ? (logn + rmax - 1) / rmax : 0;
    for (int si = 0; si < nst; si++)
      widths[si] = logn / nst + (si < logn % nst ? 1 : 0);
    return nst;
  }
  // ---- ECNTT route (ecntt.hip ecntt_run): every decision that picks a kernel or the place of its tables, from the total point
  // count tot = size * batch and the size of a point in the kernels' form (108 bytes: bn254, 168: the BLS curves) ----
  struct EcnttOverrides { // ICICLE_HIP_ECNTT_RADIX_LOG / _QUADS / _GTABS; 0 / 0 / -1 = not set
    int forced_r = 0;
    uint64_t budget = 0;
    int gtab_mode = -1; // 0 / 1 force the radix-2 stage tables into LDS / global memory, -1 auto
  };
  static inline EcnttOverrides ecntt_env_overrides() // (read once per process)
  {
    static const EcnttOverrides ov = [] {
      EcnttOverrides o;
      if (const char* s = getenv("ICICLE_HIP_ECNTT_RADIX_LOG")) o.forced_r = atoi(s);
      if (const char* s = getenv("ICICLE_HIP_ECNTT_QUADS")) o.budget = (uint64_t)atoll(s);
      if (const char* s = getenv("ICICLE_HIP_ECNTT_GTABS")) o.gtab_mode = atoi(s);
      return o;
    }();
    return ov;
  }
  struct EcnttRoute {
    uint64_t budget; // product budget of a matrix-form stage, in quads
    int nst;         // stages; widths[0 .. nst) are non-increasing and sum to logn
    int widths[64];
    int rmax;        // widths[0] (1 for a one-point transform): 1 = k_ecntt_stage (radix 2), else k_ecntt_terms + k_ecntt_sums
    bool stage_gtab; // the radix-2 stages keep their quads' 16-entry tables in global memory instead of LDS (rmax == 1 only)
    bool scale_runs; // k_ecntt_scale runs: the forward coset factors on the way in, 1 / N [and the coset] on the way out
    bool scale_gtab; // ... with its tables in global memory
  };
  // Budget: 16384 quads is the knee for transforms of up to 2^13 points (2^12: 2.04 ms against 2.71 at 32768), from 2^14 points a
  // second radix-4 stage pays (2^14: 6.49 -> 6.02 ms); profiles/r06_ecntt_quads_budget.txt. Tables: LDS holds 16 of them per
  // 64-thread block, i.e. 5 / 3 waves per CU = 20480 / 12288 quads in flight for 108 / 168-byte points; a launch with more quads
  // than that keeps them in global memory (k_ecntt_stage). A radix-2 stage has tot / 2 quads, a scale pass tot.
  static inline EcnttRoute ecntt_route(size_t point_bytes, int logn, uint64_t tot, bool inverse, bool coset, const EcnttOverrides& ov)
  {
    EcnttRoute rt;
    rt.budget = ov.budget ? ov.budget : (tot >= 16384 ? 32768 : 16384);
    rt.nst = ecntt_stage_plan(logn, tot, rt.budget, ov.forced_r, rt.widths);
    rt.rmax = rt.nst ? rt.widths[0] : 1;
    const uint64_t lds_quads = point_bytes > 120 ? 12288 : 20480;
    rt.stage_gtab = rt.rmax == 1 && (ov.gtab_mode >= 0 ? ov.gtab_mode != 0 : tot / 2 > lds_quads);
    rt.scale_runs = inverse || coset;
    rt.scale_gtab = rt.scale_runs && tot > lds_quads;
    return rt;
  }
  // exponent (mod M = 2^(q0 + r)) of the twiddle that term (j, u) of a radix-2^r stage at q0 multiplies A_j[pos] with:
  // Y[pos + L k] = sum_j w_M^(rev_r(j) (pos + L k)) A_j[pos], k = u or u + R/2 (the latter with the sign (-1)^rev_r(j))
#if defined(__HIPCC__)
  __host__ __device__
#endif
  static inline uint64_t ecntt_term_exponent(int q0, int r, uint32_t j, uint32_t u, uint64_t pos)
  {
    uint32_t rj = 0;
    for (int b = 0; b < r; b++)
      rj |= ((j >> b) & 1u) << (r - 1 - b);
    const uint64_t L = (uint64_t)1 << q0, Mmask = ((uint64_t)1 << (q0 + r)) - 1;
    return ((uint64_t)rj * (pos + L * u)) & Mmask;
  }

} // namespace icicle_hip
