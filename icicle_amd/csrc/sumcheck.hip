// Sumcheck over BabyBear, KoalaBear (one word) and the BN254, BLS12-381 scalar fields (eight words): the round kernel, and the prover,
// verifier, program and symbol functions of the reference's C ABI (src/sumcheck/sumcheck_c_api.cpp, src/program/program_c_api.cpp,
// src/symbol/symbol_api.cpp).
//
// Reference semantics: backend/cpu/include/cpu_sumcheck.h (fold of adjacent elements, round polynomial at x = 0..d), include/icicle/
// sumcheck/sumcheck.h (limits, verify), sumcheck_transcript.h (Fiat-Shamir). The host-only rules -- transcript bytes, F(digest), the
// verifier, the symbol graph and its compiler -- are in sumcheck_plan.h and program_plan.h.
//
// One round: T_r[j] = T_{r-1}[2j] + alpha (T_{r-1}[2j+1] - T_{r-1}[2j]) (r >= 1), R_r[k] = sum_i g(T_r[2i] + k (T_r[2i+1] - T_r[2i])).
// Fold, evaluate and reduce are one kernel: a lane reads the four consecutive elements of every polynomial that make one pair of T_r,
// folds them, writes the pair only while a later round will read it, and steps g through k = 0..d by adding the difference once per
// step, with d + 1 running sums per lane. Sums go lane -> wave (shuffles) -> LDS -> one partial per block; a second one-wave launch
// adds the partials. Field addition is exact, so the order of the reduction does not change a byte.
//
// Elements are canonical in memory. alpha comes in Montgomery form, so the fold's product is canonical again. The predefined programs
// convert only A and its difference: (aR) b / R - c is canonical, and E's product leaves the sum short of one factor R, which the
// second launch restores together with the last reduction (`fix`). User programs run in Montgomery form throughout.
#include "common.h"
#include "smallfield.hpp"
#include "bigfield.hpp"
#include "sumcheck_plan.h"
#include "program_device.hpp"
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>

namespace icicle_hip {

  constexpr int SC_BLOCK = 128;        // lanes of a round block (predefined programs)
  constexpr int SC_INTERP_BLOCK = 64;  // one wave: the variable file of a user program lives in LDS
  constexpr unsigned SC_MAX_GRID = 2048;
  constexpr int SC_MAX_ACC = PROG_MAX_DEGREE + 1;
  constexpr int SC_MAX_CONSTS = PROG_MAX_VARS - 2;

  struct ScPolys {
    const uint32_t* in[PROG_MAX_INPUTS]; // T_{r-1} (a folding round) or T_0 (round 0), 16-byte aligned
    uint32_t* out[PROG_MAX_INPUTS];      // T_r, written by SHAPE 1 only
  };

  // NW words (a multiple of 4) from a 16-byte aligned address
  template <int NW>
  SC_D void sc_load_words(const uint32_t* __restrict__ src, uint32_t (&w)[NW])
  {
#pragma unroll
    for (int q = 0; q < NW / 4; q++) {
      const uint4 v = reinterpret_cast<const uint4*>(src)[q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
  }
  template <int NW>
  SC_D void sc_store_words(uint32_t* __restrict__ dst, const uint32_t (&w)[NW])
  {
#pragma unroll
    for (int q = 0; q < NW / 4; q++)
      reinterpret_cast<uint4*>(dst)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }

  // SHAPE 0: the pair (T_0[2i], T_0[2i+1]) as it lies. SHAPE 1, 2: the pair of T_r folded from T_{r-1}[4i .. 4i+3]; SHAPE 1 writes it.
  template <class FA, int SHAPE>
  SC_D void sc_load_pair(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t i, const typename FA::elem& alpha, typename FA::elem& lo,
                         typename FA::elem& hi)
  {
    using elem = typename FA::elem;
    if constexpr (FA::W == 1) {
      if constexpr (SHAPE == 0) {
        const uint2 v = reinterpret_cast<const uint2*>(in)[i];
        lo = v.x, hi = v.y;
      } else {
        const uint4 v = reinterpret_cast<const uint4*>(in)[i];
        lo = FA::add(v.x, FA::mul(FA::sub(v.y, v.x), alpha));
        hi = FA::add(v.z, FA::mul(FA::sub(v.w, v.z), alpha));
        if constexpr (SHAPE == 1) reinterpret_cast<uint2*>(out)[i] = make_uint2(lo, hi);
      }
    } else if constexpr (SHAPE == 0) {
      uint32_t w[2 * FA::W];
      sc_load_words(in + 2 * FA::W * i, w);
      lo = FA::load(w), hi = FA::load(w + FA::W);
    } else {
      uint32_t w[4 * FA::W];
      sc_load_words(in + 4 * FA::W * i, w);
      const elem e0 = FA::load(w), e1 = FA::load(w + FA::W), e2 = FA::load(w + 2 * FA::W), e3 = FA::load(w + 3 * FA::W);
      lo = FA::add(e0, FA::mul(FA::sub(e1, e0), alpha));
      hi = FA::add(e2, FA::mul(FA::sub(e3, e2), alpha));
      if constexpr (SHAPE == 1) {
        uint32_t o[2 * FA::W];
        FA::store(o, lo), FA::store(o + FA::W, hi);
        sc_store_words(out + 2 * FA::W * i, o);
      }
    }
  }

  // acc[k] of every lane of the block summed into partial[k]; NACC compile-time slots of which `count` are in use
  template <class FA, int NACC, int BLOCK>
  SC_D void sc_block_reduce(typename FA::elem (&acc)[NACC], int count, typename FA::elem* __restrict__ partial)
  {
    using elem = typename FA::elem;
    constexpr int WAVES = BLOCK / 64;
    __shared__ uint32_t smem[WAVES * NACC * FA::REGS];
#pragma unroll
    for (int k = 0; k < NACC; k++) {
      if (k >= count) break;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        elem o;
#pragma unroll
        for (int q = 0; q < FA::REGS; q++)
          FA::reg(o, q) = (uint32_t)__shfl_down((int)FA::reg(acc[k], q), off);
        acc[k] = FA::add(acc[k], o);
      }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (WAVES > 1) {
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NACC; k++)
#pragma unroll
          for (int q = 0; q < FA::REGS; q++)
            smem[(wave * NACC + k) * FA::REGS + q] = FA::reg(acc[k], q);
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < NACC; k++) {
        if (k >= count) break;
        elem s = acc[k];
        if constexpr (WAVES > 1) {
          for (int v = 1; v < WAVES; v++) {
            elem o;
#pragma unroll
            for (int q = 0; q < FA::REGS; q++)
              FA::reg(o, q) = smem[(v * NACC + k) * FA::REGS + q];
            s = FA::add(s, o);
          }
        }
        partial[k] = s;
      }
    }
  }

  // ---- the predefined programs -------------------------------------------------------------------------------------------------------
  template <class FA, int PROG>
  struct ScPredef;
  template <class FA>
  struct ScPredef<FA, PROG_AB_MINUS_C> { // A B - C
    using elem = typename FA::elem;
    static constexpr int M = 3, D = 2;
    static elem fix() { return FA::mont_one(); } // the sums are canonical already
    static SC_D void accumulate(const elem (&lo)[M], const elem (&hi)[M], elem (&acc)[D + 1])
    {
      elem a = FA::mul(lo[0], FA::r2()), da = FA::mul(FA::sub(hi[0], lo[0]), FA::r2());
      elem b = lo[1], c = lo[2];
      const elem db = FA::sub(hi[1], lo[1]), dc = FA::sub(hi[2], lo[2]);
#pragma unroll
      for (int k = 0; k <= D; k++) {
        acc[k] = FA::add(acc[k], FA::sub(FA::mul(a, b), c));
        if (k < D) a = FA::add(a, da), b = FA::add(b, db), c = FA::add(c, dc);
      }
    }
  };
  template <class FA>
  struct ScPredef<FA, PROG_EQ_X_AB_MINUS_C> { // E (A B - C)
    using elem = typename FA::elem;
    static constexpr int M = 4, D = 3;
    static elem fix() { return FA::r2(); } // the sums carry 1 / R
    static SC_D void accumulate(const elem (&lo)[M], const elem (&hi)[M], elem (&acc)[D + 1])
    {
      elem a = FA::mul(lo[0], FA::r2()), da = FA::mul(FA::sub(hi[0], lo[0]), FA::r2());
      elem b = lo[1], c = lo[2], e = lo[3];
      const elem db = FA::sub(hi[1], lo[1]), dc = FA::sub(hi[2], lo[2]), de = FA::sub(hi[3], lo[3]);
#pragma unroll
      for (int k = 0; k <= D; k++) {
        acc[k] = FA::add(acc[k], FA::mul(e, FA::sub(FA::mul(a, b), c)));
        if (k < D) a = FA::add(a, da), b = FA::add(b, db), c = FA::add(c, dc), e = FA::add(e, de);
      }
    }
  };

  // `pairs` = |T_r| / 2 >= 1. partials: gridDim.x rows of D + 1 elements.
  template <class PR, int PROG, int SHAPE>
  __global__ __launch_bounds__(SC_BLOCK) void k_sumcheck_round(ScPolys p, typename ScFieldOf<PR>::type::elem alpha, uint64_t pairs,
                                                               typename ScFieldOf<PR>::type::elem* __restrict__ partials)
  {
    using FA = typename ScFieldOf<PR>::type;
    using PG = ScPredef<FA, PROG>;
    using elem = typename FA::elem;
    constexpr int M = PG::M, NACC = PG::D + 1;
    elem acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; k++)
      acc[k] = FA::zero();
    const uint64_t stride = (uint64_t)gridDim.x * SC_BLOCK, first = (uint64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if constexpr (FA::W == 1 && SHAPE == 0) {
      // two pairs per 16-byte load; the one-pair table (n = 2) is the only odd size
      for (uint64_t t = first; t < pairs / 2; t += stride) {
        elem lo[2][M], hi[2][M];
#pragma unroll
        for (int j = 0; j < M; j++) {
          const uint4 v = reinterpret_cast<const uint4*>(p.in[j])[t];
          lo[0][j] = v.x, hi[0][j] = v.y, lo[1][j] = v.z, hi[1][j] = v.w;
        }
        PG::accumulate(lo[0], hi[0], acc);
        PG::accumulate(lo[1], hi[1], acc);
      }
      if (pairs == 1 && first == 0) {
        elem lo[M], hi[M];
#pragma unroll
        for (int j = 0; j < M; j++)
          sc_load_pair<FA, 0>(p.in[j], nullptr, 0, alpha, lo[j], hi[j]);
        PG::accumulate(lo, hi, acc);
      }
    } else {
      for (uint64_t i = first; i < pairs; i += stride) {
        elem lo[M], hi[M];
#pragma unroll
        for (int j = 0; j < M; j++)
          sc_load_pair<FA, SHAPE>(p.in[j], p.out[j], i, alpha, lo[j], hi[j]);
        PG::accumulate(lo, hi, acc);
      }
    }
    sc_block_reduce<FA, NACC, SC_BLOCK>(acc, NACC, partials + (size_t)blockIdx.x * NACC);
  }

  // ---- user programs: an interpreter over the compiled instruction list ------------------------------------------------------------
  template <class FA>
  struct ScProgramArgs {
    int nof_inputs, nof_parameters, nof_constants, nof_ins, degree;
    uint32_t ins[PROG_MAX_VARS]; // op | a << 8 | b << 16 | dst << 24; at most one instruction per variable
    typename FA::elem constants[SC_MAX_CONSTS]; // Montgomery form
  };

  // The variable file of a lane: PROG_MAX_VARS variables, then the differences of the inputs; word q of slot s of lane l at
  // [(s REGS + q) 64 + l], so the lanes of a wave read consecutive words.
  template <class FA>
  struct ScVars {
    static constexpr int SLOTS = PROG_MAX_VARS + PROG_MAX_INPUTS;
    uint32_t* base;
    SC_D typename FA::elem ld(int slot) const
    {
      typename FA::elem e;
#pragma unroll
      for (int q = 0; q < FA::REGS; q++)
        FA::reg(e, q) = base[(slot * FA::REGS + q) * SC_INTERP_BLOCK];
      return e;
    }
    SC_D void st(int slot, typename FA::elem e) const
    {
#pragma unroll
      for (int q = 0; q < FA::REGS; q++)
        base[(slot * FA::REGS + q) * SC_INTERP_BLOCK] = FA::reg(e, q);
    }
  };

  template <class PR, int SHAPE>
  __global__ __launch_bounds__(SC_INTERP_BLOCK) void k_sumcheck_round_program(ScPolys p, typename ScFieldOf<PR>::type::elem alpha, uint64_t pairs,
                                                                              typename ScFieldOf<PR>::type::elem* __restrict__ partials,
                                                                              ScProgramArgs<typename ScFieldOf<PR>::type> g)
  {
    using FA = typename ScFieldOf<PR>::type;
    using elem = typename FA::elem;
    __shared__ uint32_t file[ScVars<FA>::SLOTS * FA::REGS * SC_INTERP_BLOCK];
    const ScVars<FA> v{file + threadIdx.x};
    elem acc[SC_MAX_ACC];
#pragma unroll
    for (int k = 0; k < SC_MAX_ACC; k++)
      acc[k] = FA::zero();
    for (int c = 0; c < g.nof_constants; c++)
      v.st(g.nof_parameters + c, g.constants[c]);
    const uint64_t stride = (uint64_t)gridDim.x * SC_INTERP_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * SC_INTERP_BLOCK + threadIdx.x; i < pairs; i += stride) {
      for (int j = 0; j < g.nof_inputs; j++) {
        elem lo, hi;
        sc_load_pair<FA, SHAPE>(p.in[j], p.out[j], i, alpha, lo, hi);
        v.st(j, FA::mul(lo, FA::r2()));
        v.st(PROG_MAX_VARS + j, FA::mul(FA::sub(hi, lo), FA::r2()));
      }
#pragma unroll
      for (int k = 0; k < SC_MAX_ACC; k++) {
        if (k > g.degree) break;
        for (int q = 0; q < g.nof_ins; q++) {
          const uint32_t ins = g.ins[q];
          const elem a = v.ld((ins >> 8) & 0xff), b = v.ld((ins >> 16) & 0xff);
          const uint32_t op = ins & 0xff;
          v.st(ins >> 24, op == PROG_MUL ? FA::mul(a, b) : op == PROG_ADD ? FA::add(a, b) : op == PROG_SUB ? FA::sub(a, b) : a);
        }
        acc[k] = FA::add(acc[k], v.ld(g.nof_inputs));
        if (k < g.degree)
          for (int j = 0; j < g.nof_inputs; j++)
            v.st(j, FA::add(v.ld(j), v.ld(PROG_MAX_VARS + j)));
      }
    }
    sc_block_reduce<FA, SC_MAX_ACC, SC_INTERP_BLOCK>(acc, g.degree + 1, partials + (size_t)blockIdx.x * SC_MAX_ACC);
  }

  // one wave: out[k] = fix * sum over the rows of partials[row][k], canonical words; `pitch` elements per row
  template <class PR>
  __global__ __launch_bounds__(64) void k_sumcheck_finish(const typename ScFieldOf<PR>::type::elem* __restrict__ partials, uint32_t rows, int pitch, int count,
                                                          typename ScFieldOf<PR>::type::elem fix, uint32_t* __restrict__ out)
  {
    using FA = typename ScFieldOf<PR>::type;
    using elem = typename FA::elem;
    for (int k = 0; k < count; k++) {
      elem s = FA::zero();
      for (uint32_t r = threadIdx.x; r < rows; r += 64)
        s = FA::add(s, partials[(size_t)r * pitch + k]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        elem o;
#pragma unroll
        for (int q = 0; q < FA::REGS; q++)
          FA::reg(o, q) = (uint32_t)__shfl_down((int)FA::reg(s, q), off);
        s = FA::add(s, o);
      }
      if (threadIdx.x == 0) FA::store(out + k * FA::W, FA::mul(s, fix));
    }
  }

  // ---- objects behind the handles ----------------------------------------------------------------------------------------------------
  struct SymbolObj {
    int words = 0;
    SymRef node;
  };
  struct SumcheckObj {
    std::vector<uint32_t> challenge; // alpha_0 = 0, alpha_1, ..: one element per round of the last proof
  };
  struct SumcheckProofObj {
    std::vector<std::vector<uint32_t>> polys; // round polynomials, d + 1 elements each
  };

  // Symbols made through the C ABI belong to the library until the next generate_*_program, which frees all of them (the
  // reference's ReleasePool).
  static std::mutex g_symbol_mtx;
  static std::vector<SymbolObj*> g_symbols;
  static icicle_symbol_handle_t symbol_new(int words, SymRef node)
  {
    SymbolObj* s = new SymbolObj{words, std::move(node)};
    std::lock_guard<std::mutex> lk(g_symbol_mtx);
    g_symbols.push_back(s);
    return (icicle_symbol_handle_t)s;
  }
  static void symbols_release()
  {
    std::lock_guard<std::mutex> lk(g_symbol_mtx);
    for (SymbolObj* s : g_symbols)
      delete s;
    g_symbols.clear();
  }
  static icicle_error_t symbol_binary(int words, ProgOp op, icicle_symbol_handle_t a, icicle_symbol_handle_t b, icicle_symbol_handle_t* res)
  {
    if (!a || !b) return ICICLE_INVALID_ARGUMENT; // the reference's codes (symbol_api.cpp)
    if (!res) return ICICLE_INVALID_POINTER;
    const SymbolObj *x = (const SymbolObj*)a, *y = (const SymbolObj*)b;
    if (x->words != words || y->words != words) return ICICLE_INVALID_ARGUMENT;
    *res = symbol_new(words, sym_op(op, x->node, y->node));
    return ICICLE_SUCCESS;
  }
  static icicle_error_t symbol_inverse(int words, icicle_symbol_handle_t a, icicle_symbol_handle_t* res)
  {
    if (!a || !res) return ICICLE_INVALID_POINTER;
    const SymbolObj* x = (const SymbolObj*)a;
    if (x->words != words) return ICICLE_INVALID_ARGUMENT;
    *res = symbol_new(words, sym_op(PROG_INV, x->node, nullptr));
    return ICICLE_SUCCESS;
  }
  // general: a program with any number of outputs (<field>_generate_program), else the last parameter is the return value
  static icicle_error_t program_generate(int words, icicle_symbol_handle_t* params, int nof_parameters, icicle_program_handle_t* program, bool general = false)
  {
    if (!params || !program) return ICICLE_INVALID_POINTER;
    *program = nullptr;
    if (nof_parameters < 1) return ICICLE_INVALID_ARGUMENT;
    std::vector<SymRef> nodes;
    for (int i = 0; i < nof_parameters; i++) {
      const SymbolObj* s = (const SymbolObj*)params[i];
      if (!s || s->words != words) return ICICLE_INVALID_ARGUMENT;
      nodes.push_back(s->node);
    }
    std::unique_ptr<ProgramObj> obj(new ProgramObj);
    obj->words = words;
    const bool ok = ProgramCompiler().run(nodes, words, &obj->prog, general);
    symbols_release();
    if (!ok) return ICICLE_INVALID_ARGUMENT;
    *program = (icicle_program_handle_t)obj.release();
    return ICICLE_SUCCESS;
  }

  static icicle_error_t transcript_hash(icicle_hasher_handle_t hasher, const std::vector<uint8_t>& msg, hipStream_t st, std::vector<uint8_t>* digest)
  {
    if (msg.empty()) return ICICLE_INVALID_ARGUMENT;
    digest->assign(icicle_hasher_output_size(hasher), 0);
    icicle_hash_config_t hc{};
    hc.stream = (icicleStreamHandle)st, hc.batch = 1;
    return icicle_hasher_hash(hasher, msg.data(), msg.size(), &hc, digest->data());
  }
  static SumcheckLabels labels_of(const icicle_sumcheck_transcript_config_t* t)
  {
    return SumcheckLabels{t->domain_separator_label,     t->round_poly_label,     t->round_challenge_label,
                          t->domain_separator_label_len, t->round_poly_label_len, t->round_challenge_label_len};
  }

  template <class FA>
  static typename FA::elem to_mont_host(const uint32_t* canonical)
  {
    return FA::mul(FA::load(canonical), FA::r2());
  }

  // ---- per-round device times of the last proof, for tools/sumcheck_bench.py (icicle_hip_sumcheck_time_rounds) ----
  static std::atomic<bool> g_time_rounds{false};
  static std::mutex g_round_times_mtx;
  static std::vector<double> g_round_times; // ms, the round kernel and the second launch together
  struct RoundTimer {
    hipEvent_t a = nullptr, b = nullptr;
    bool on = false;
    explicit RoundTimer(bool enable) : on(enable && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) {}
    RoundTimer(const RoundTimer&) = delete;
    RoundTimer& operator=(const RoundTimer&) = delete;
    ~RoundTimer()
    {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
    void begin(hipStream_t st)
    {
      if (on) (void)hipEventRecord(a, st);
    }
    void end(hipStream_t st)
    {
      if (on) (void)hipEventRecord(b, st);
    }
    void read(std::vector<double>* out) // after the stream is drained
    {
      float ms = 0;
      if (on && hipEventElapsedTime(&ms, a, b) == hipSuccess) out->push_back(ms);
    }
  };

  template <class PR, int SHAPE>
  static void launch_round(const CompiledProgram& g, const ScProgramArgs<typename ScFieldOf<PR>::type>& args, unsigned grid, const ScPolys& p,
                           const typename ScFieldOf<PR>::type::elem& alpha, uint64_t pairs, typename ScFieldOf<PR>::type::elem* partials, hipStream_t st)
  {
    if (g.predefined == PROG_AB_MINUS_C)
      k_sumcheck_round<PR, PROG_AB_MINUS_C, SHAPE><<<grid, SC_BLOCK, 0, st>>>(p, alpha, pairs, partials);
    else if (g.predefined == PROG_EQ_X_AB_MINUS_C)
      k_sumcheck_round<PR, PROG_EQ_X_AB_MINUS_C, SHAPE><<<grid, SC_BLOCK, 0, st>>>(p, alpha, pairs, partials);
    else
      k_sumcheck_round_program<PR, SHAPE><<<grid, SC_INTERP_BLOCK, 0, st>>>(p, alpha, pairs, partials, args);
  }

  template <class PR>
  static icicle_error_t sumcheck_prove(SumcheckObj* sc, const uint32_t* const* polys, uint64_t n, uint64_t nof_polys, const uint32_t* claimed_sum, const ProgramObj* program,
                                       const icicle_sumcheck_transcript_config_t* tc, const icicle_sumcheck_config_t* cfg, SumcheckProofObj* proof)
  {
    using FA = typename ScFieldOf<PR>::type;
    using elem = typename FA::elem;
    constexpr size_t EB = 4 * FA::W;
    if (!sc || !polys || !claimed_sum || !program || !tc || !tc->hasher || !tc->seed_rng || !cfg || !proof) return ICICLE_INVALID_POINTER;
    if (cfg->use_extension_field || program->words != FA::W) return ICICLE_INVALID_ARGUMENT;
    if (n < 2 || !sumcheck_is_pow2(n) || n > ((uint64_t)1 << 40)) return ICICLE_INVALID_ARGUMENT;
    const CompiledProgram& g = program->prog;
    if (program_check_for_sumcheck(g, nof_polys)) return ICICLE_INVALID_ARGUMENT;
    const int m = (int)nof_polys, d = g.degree;
    for (int j = 0; j < m; j++)
      if (!polys[j]) return ICICLE_INVALID_POINTER;
    const uint32_t L = sumcheck_log2(n);
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    // ext "hip_sumcheck_max_grid" (int): fewer blocks per round launch, so that small sizes walk the grid more than once (a test
    // hook). Absent or <= 0: SC_MAX_GRID, which is also the most, as the partials are sized by it.
    const int grid_key = cfg->ext ? reinterpret_cast<const ConfigExt*>(cfg->ext)->get_int("hip_sumcheck_max_grid", 0) : 0;
    const unsigned max_grid = grid_key <= 0 ? SC_MAX_GRID : std::min<unsigned>((unsigned)grid_key, SC_MAX_GRID);

    // T_0 where the caller has it when that is 16-byte aligned device memory, else a copy; T_r alternates between two scratch
    // tables of n / 2 and n / 4 elements per polynomial. The caller's polynomials are never written.
    bool copy_in = !cfg->are_inputs_on_device;
    for (int j = 0; j < m; j++)
      copy_in = copy_in || ((uintptr_t)polys[j] & 15) != 0;
    const auto pitch = [&](uint64_t elems) { return (size_t)((elems * EB + 15) & ~(uint64_t)15); };
    TempBuf d_in, d_a, d_b, d_partials, d_out;
    ScPolys t0{}, ta{}, tb{};
    if (copy_in) HIP_TRY(d_in.alloc(pitch(n) * m, st), ICICLE_ALLOCATION_FAILED);
    if (L >= 3) HIP_TRY(d_a.alloc(pitch(n / 2) * m, st), ICICLE_ALLOCATION_FAILED);
    if (L >= 4) HIP_TRY(d_b.alloc(pitch(n / 4) * m, st), ICICLE_ALLOCATION_FAILED);
    for (int j = 0; j < m; j++) {
      if (copy_in) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(d_in.as<uint8_t>() + pitch(n) * j);
        HIP_TRY(hipMemcpyAsync(dst, polys[j], n * EB, cfg->are_inputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
        t0.in[j] = dst;
      } else {
        t0.in[j] = polys[j];
      }
      if (L >= 3) ta.out[j] = reinterpret_cast<uint32_t*>(d_a.as<uint8_t>() + pitch(n / 2) * j);
      if (L >= 4) tb.out[j] = reinterpret_cast<uint32_t*>(d_b.as<uint8_t>() + pitch(n / 4) * j);
    }
    HIP_TRY(d_partials.alloc((size_t)SC_MAX_GRID * SC_MAX_ACC * sizeof(elem), st), ICICLE_ALLOCATION_FAILED);
    HIP_TRY(d_out.alloc(SC_MAX_ACC * EB, st), ICICLE_ALLOCATION_FAILED);

    ScProgramArgs<FA> args{};
    elem fix = FA::plain_one(); // a user program's sums are in Montgomery form
    int acc_pitch = SC_MAX_ACC, block = SC_INTERP_BLOCK;
    if (g.predefined >= 0) {
      fix = g.predefined == PROG_AB_MINUS_C ? ScPredef<FA, PROG_AB_MINUS_C>::fix() : ScPredef<FA, PROG_EQ_X_AB_MINUS_C>::fix();
      acc_pitch = d + 1, block = SC_BLOCK;
    } else {
      if (g.ins.size() > (size_t)PROG_MAX_VARS || g.nof_constants > SC_MAX_CONSTS) return ICICLE_INVALID_ARGUMENT;
      args.nof_inputs = m, args.nof_parameters = g.nof_parameters, args.nof_constants = g.nof_constants, args.nof_ins = (int)g.ins.size(), args.degree = d;
      for (size_t q = 0; q < g.ins.size(); q++) {
        const ProgInstr& in = g.ins[q];
        if (in.op > PROG_SUB || in.a >= g.nof_vars() || in.b >= g.nof_vars() || in.dst >= g.nof_vars() || in.dst < m) return ICICLE_INVALID_ARGUMENT;
        args.ins[q] = (uint32_t)in.op | (uint32_t)in.a << 8 | (uint32_t)in.b << 16 | (uint32_t)in.dst << 24;
      }
      for (int c = 0; c < g.nof_constants; c++)
        args.constants[c] = to_mont_host<FA>(g.constants[c].data());
    }

    const SumcheckTranscriptBytes transcript(labels_of(tc), L, (uint32_t)d, reinterpret_cast<const uint8_t*>(claimed_sum), reinterpret_cast<const uint8_t*>(tc->seed_rng), EB);
    const HostField hf = FA::host_field();
    std::vector<std::vector<uint32_t>> round_polys(L, std::vector<uint32_t>((size_t)(d + 1) * FA::W, 0));
    std::vector<uint32_t> challenge((size_t)L * FA::W, 0);
    std::vector<uint8_t> digest;
    RoundTimer timer(g_time_rounds.load(std::memory_order_relaxed));
    std::vector<double> times;
    for (uint32_t r = 0; r < L; r++) {
      uint32_t* alpha = &challenge[(size_t)r * FA::W]; // alpha_0 = 0 is recorded and never used
      if (r > 0) {
        const uint8_t* prev = reinterpret_cast<const uint8_t*>(&challenge[(size_t)(r - 1) * FA::W]);
        ICICLE_TRY(transcript_hash(tc->hasher, transcript.round_input(r - 1, prev, reinterpret_cast<const uint8_t*>(round_polys[r - 1].data())), st, &digest));
        hf.from_digest(digest.data(), digest.size(), alpha);
      }
      const elem alpha_m = to_mont_host<FA>(alpha);
      const uint64_t pairs = n >> (r + 1);
      const bool store = r >= 1 && r + 1 < L; // a later round reads T_r
      // round r >= 1 reads T_{r-1}: the input (r = 1), table a (r even), table b (r odd, >= 3); it writes the other table
      ScPolys p{};
      for (int j = 0; j < m; j++) {
        p.in[j] = r <= 1 ? t0.in[j] : (r % 2 == 0 ? ta.out[j] : tb.out[j]);
        p.out[j] = !store ? nullptr : (r % 2 == 1 ? ta.out[j] : tb.out[j]);
      }
      const uint64_t items = (FA::W == 1 && r == 0 && g.predefined >= 0 && pairs > 1) ? pairs / 2 : pairs;
      const unsigned grid = (unsigned)std::min<uint64_t>((items + block - 1) / block, max_grid);
      elem* partials = d_partials.as<elem>();
      timer.begin(st);
      if (r == 0)
        launch_round<PR, 0>(g, args, grid, p, alpha_m, pairs, partials, st);
      else if (store)
        launch_round<PR, 1>(g, args, grid, p, alpha_m, pairs, partials, st);
      else
        launch_round<PR, 2>(g, args, grid, p, alpha_m, pairs, partials, st);
      LAUNCH_CHECK("k_sumcheck_round", st);
      k_sumcheck_finish<PR><<<1, 64, 0, st>>>(partials, grid, acc_pitch, d + 1, fix, d_out.as<uint32_t>());
      LAUNCH_CHECK("k_sumcheck_finish", st);
      timer.end(st);
      HIP_TRY(hipMemcpyAsync(round_polys[r].data(), d_out.ptr(), (size_t)(d + 1) * EB, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
      HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED); // the next challenge is derived on the host
      timer.read(&times);
    }
    if (timer.on) {
      std::lock_guard<std::mutex> lk(g_round_times_mtx);
      g_round_times.swap(times);
    }
    proof->polys.swap(round_polys);
    sc->challenge.swap(challenge);
    return ICICLE_SUCCESS;
  }

  template <class PR>
  static icicle_error_t sumcheck_verify(const SumcheckProofObj* proof, const uint32_t* claimed_sum, const icicle_sumcheck_transcript_config_t* tc, bool* valid)
  {
    using FA = typename ScFieldOf<PR>::type;
    if (!proof || !claimed_sum || !tc || !tc->hasher || !tc->seed_rng || !valid) return ICICLE_INVALID_POINTER;
    *valid = false;
    const uint64_t rounds = proof->polys.size(), size = rounds ? proof->polys[0].size() / FA::W : 0;
    std::vector<uint32_t> flat;
    for (const auto& rp : proof->polys) {
      if (rp.size() != size * FA::W) return ICICLE_SUCCESS; // round polynomials of different lengths: a wrong proof
      flat.insert(flat.end(), rp.begin(), rp.end());
    }
    icicle_error_t err = ICICLE_SUCCESS;
    bool bound = false;
    const SumcheckHashFn hash = [&](const std::vector<uint8_t>& msg, std::vector<uint8_t>* digest) {
      if (!bound) err = bind_current_device(), bound = true;
      if (err == ICICLE_SUCCESS) err = transcript_hash(tc->hasher, msg, nullptr, digest);
      return err == ICICLE_SUCCESS;
    };
    if (sumcheck_verify_host(FA::host_field(), flat.data(), rounds, size, claimed_sum, tc->seed_rng, labels_of(tc), hash, valid)) {
      *valid = false;
      return err != ICICLE_SUCCESS ? err : ICICLE_INVALID_ARGUMENT;
    }
    return ICICLE_SUCCESS;
  }

  static SumcheckProofObj* proof_from_polys(uint32_t** polys, uint64_t nof_polynomials, uint64_t poly_size, int words)
  {
    if (nof_polynomials && !polys) return nullptr;
    std::unique_ptr<SumcheckProofObj> p(new SumcheckProofObj);
    for (uint64_t i = 0; i < nof_polynomials; i++) {
      if (!polys[i]) return nullptr;
      p->polys.emplace_back(polys[i], polys[i] + poly_size * words);
    }
    return p.release();
  }

} // namespace icicle_hip

using namespace icicle_hip;

static_assert(sizeof(icicle_sumcheck_config_t) == 40 && offsetof(icicle_sumcheck_config_t, use_extension_field) == 8 && offsetof(icicle_sumcheck_config_t, batch) == 16 &&
                offsetof(icicle_sumcheck_config_t, are_inputs_on_device) == 24 && offsetof(icicle_sumcheck_config_t, is_async) == 25 &&
                offsetof(icicle_sumcheck_config_t, ext) == 32,
              "SumcheckConfig layout (include/icicle/sumcheck/sumcheck_config.h)");
static_assert(sizeof(icicle_sumcheck_transcript_config_t) == 72 && offsetof(icicle_sumcheck_transcript_config_t, little_endian) == 56 &&
                offsetof(icicle_sumcheck_transcript_config_t, seed_rng) == 64,
              "TranscriptConfigFFI layout (src/sumcheck/sumcheck_c_api.cpp)");

#define SC_GUARDED(expr)                                                                                               \
  try {                                                                                                                \
    return (expr);                                                                                                     \
  } catch (...) {                                                                                                      \
    return ICICLE_ALLOCATION_FAILED;                                                                                   \
  }

extern "C" icicle_error_t icicle_hip_sumcheck_time_rounds(bool enable)
{
  g_time_rounds.store(enable);
  return ICICLE_SUCCESS;
}
extern "C" icicle_error_t icicle_hip_sumcheck_round_times(double* ms, int capacity, int* rounds)
{
  if (!ms || !rounds) return ICICLE_INVALID_POINTER;
  std::lock_guard<std::mutex> lk(g_round_times_mtx);
  *rounds = (int)g_round_times.size();
  for (int i = 0; i < capacity && i < *rounds; i++)
    ms[i] = g_round_times[i];
  return ICICLE_SUCCESS;
}

extern "C" icicle_error_t icicle_hip_sumcheck_launch_info(int predefined, int* block, int* max_grid)
{
  if (!block || !max_grid) return ICICLE_INVALID_POINTER;
  *block = predefined ? SC_BLOCK : SC_INTERP_BLOCK;
  *max_grid = (int)SC_MAX_GRID;
  return ICICLE_SUCCESS;
}

extern "C" icicle_error_t delete_program(icicle_program_handle_t program)
{
  if (!program) return ICICLE_INVALID_POINTER;
  delete (ProgramObj*)program;
  return ICICLE_SUCCESS;
}

#define DEFINE_SUMCHECK(P, PR)                                                                                         \
  extern "C" icicle_sumcheck_handle_t P##_sumcheck_create(void) { return (icicle_sumcheck_handle_t) new (std::nothrow) SumcheckObj; } \
  extern "C" icicle_error_t P##_sumcheck_delete(icicle_sumcheck_handle_t sumcheck)                                     \
  {                                                                                                                    \
    if (!sumcheck) return ICICLE_INVALID_ARGUMENT;                                                                     \
    delete (SumcheckObj*)sumcheck;                                                                                     \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_hip_sumcheck_prove(icicle_sumcheck_handle_t sumcheck, const uint32_t* const* mle_polynomials, uint64_t mle_polynomial_size, \
                                                   uint64_t nof_mle_polynomials, const uint32_t* claimed_sum, icicle_program_handle_t combine_function, \
                                                   const icicle_sumcheck_transcript_config_t* transcript_config, const icicle_sumcheck_config_t* sumcheck_config, \
                                                   icicle_sumcheck_proof_handle_t proof)                               \
  {                                                                                                                    \
    SC_GUARDED((sumcheck_prove<PR>((SumcheckObj*)sumcheck, mle_polynomials, mle_polynomial_size, nof_mle_polynomials, claimed_sum, (const ProgramObj*)combine_function, \
                                   transcript_config, sumcheck_config, (SumcheckProofObj*)proof)))                     \
  }                                                                                                                    \
  extern "C" icicle_sumcheck_proof_handle_t P##_sumcheck_get_proof(icicle_sumcheck_handle_t sumcheck, const uint32_t* const* mle_polynomials,                  \
                                                                   uint64_t mle_polynomial_size, uint64_t nof_mle_polynomials, const uint32_t* claimed_sum,    \
                                                                   icicle_program_handle_t combine_function,           \
                                                                   const icicle_sumcheck_transcript_config_t* transcript_config,                               \
                                                                   const icicle_sumcheck_config_t* sumcheck_config)    \
  {                                                                                                                    \
    SumcheckProofObj* proof = new (std::nothrow) SumcheckProofObj;                                                     \
    if (!proof) return nullptr;                                                                                        \
    if (P##_hip_sumcheck_prove(sumcheck, mle_polynomials, mle_polynomial_size, nof_mle_polynomials, claimed_sum, combine_function, transcript_config, sumcheck_config, \
                               (icicle_sumcheck_proof_handle_t)proof) != ICICLE_SUCCESS) {                            \
      delete proof;                                                                                                    \
      return nullptr;                                                                                                  \
    }                                                                                                                  \
    return (icicle_sumcheck_proof_handle_t)proof;                                                                      \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_sumcheck_verify(icicle_sumcheck_handle_t sumcheck, icicle_sumcheck_proof_handle_t proof, const uint32_t* claimed_sum,         \
                                                const icicle_sumcheck_transcript_config_t* transcript_config, bool* is_verified)                              \
  {                                                                                                                    \
    if (!sumcheck) return ICICLE_INVALID_POINTER;                                                                      \
    SC_GUARDED((sumcheck_verify<PR>((const SumcheckProofObj*)proof, claimed_sum, transcript_config, is_verified)))     \
  }                                                                                                                    \
  extern "C" icicle_sumcheck_proof_handle_t P##_sumcheck_proof_create(uint32_t** polys, uint64_t nof_polynomials, uint64_t poly_size)                         \
  {                                                                                                                    \
    try {                                                                                                              \
      return (icicle_sumcheck_proof_handle_t)proof_from_polys(polys, nof_polynomials, poly_size, ScFieldOf<PR>::type::W);                                     \
    } catch (...) {                                                                                                    \
      return nullptr;                                                                                                  \
    }                                                                                                                  \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_sumcheck_proof_get_poly_sizes(icicle_sumcheck_proof_handle_t proof, uint64_t* poly_size, uint64_t* nof_polys)                 \
  {                                                                                                                    \
    if (!proof) return ICICLE_INVALID_ARGUMENT;                                                                        \
    if (!poly_size || !nof_polys) return ICICLE_INVALID_POINTER;                                                       \
    const SumcheckProofObj* p = (const SumcheckProofObj*)proof;                                                        \
    *nof_polys = p->polys.size();                                                                                      \
    *poly_size = p->polys.empty() ? 0 : p->polys[0].size() / ScFieldOf<PR>::type::W;                                   \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" uint32_t* P##_sumcheck_proof_get_round_poly_at(icicle_sumcheck_proof_handle_t proof, uint64_t index)      \
  {                                                                                                                    \
    SumcheckProofObj* p = (SumcheckProofObj*)proof;                                                                    \
    return (!p || index >= p->polys.size()) ? nullptr : p->polys[index].data();                                        \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_sumcheck_proof_delete(icicle_sumcheck_proof_handle_t proof)                            \
  {                                                                                                                    \
    if (!proof) return ICICLE_INVALID_ARGUMENT;                                                                        \
    delete (SumcheckProofObj*)proof;                                                                                   \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_sumcheck_get_challenge_size(icicle_sumcheck_handle_t sumcheck, size_t* challenge_size) \
  {                                                                                                                    \
    if (!sumcheck) return ICICLE_INVALID_ARGUMENT;                                                                     \
    if (!challenge_size) return ICICLE_INVALID_POINTER;                                                                \
    *challenge_size = ((const SumcheckObj*)sumcheck)->challenge.size() / ScFieldOf<PR>::type::W;                       \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_sumcheck_get_challenge_vector(icicle_sumcheck_handle_t sumcheck, uint32_t* challenge_vector, size_t* challenge_vector_size)   \
  {                                                                                                                    \
    if (!sumcheck || !challenge_vector_size) return ICICLE_INVALID_ARGUMENT;                                           \
    if (!challenge_vector) return ICICLE_INVALID_POINTER;                                                              \
    const SumcheckObj* s = (const SumcheckObj*)sumcheck;                                                               \
    const size_t have = s->challenge.size() / ScFieldOf<PR>::type::W;                                                  \
    if (*challenge_vector_size > have) *challenge_vector_size = have;                                                  \
    std::memcpy(challenge_vector, s->challenge.data(), *challenge_vector_size * 4 * ScFieldOf<PR>::type::W);           \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_program_handle_t P##_create_predefined_returning_value_program(int pre_def)                        \
  {                                                                                                                    \
    ProgramObj* obj = new (std::nothrow) ProgramObj;                                                                   \
    if (!obj) return nullptr;                                                                                          \
    obj->words = ScFieldOf<PR>::type::W;                                                                               \
    if (!program_predefined(pre_def, &obj->prog)) {                                                                    \
      delete obj;                                                                                                      \
      return nullptr;                                                                                                  \
    }                                                                                                                  \
    return (icicle_program_handle_t)obj;                                                                               \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_generate_returning_value_program(icicle_symbol_handle_t* parameters, int nof_parameters, icicle_program_handle_t* program)    \
  {                                                                                                                    \
    SC_GUARDED(program_generate(ScFieldOf<PR>::type::W, parameters, nof_parameters, program))                          \
  }                                                                                                                    \
  extern "C" icicle_program_handle_t P##_create_predefined_program(int pre_def)                                        \
  {                                                                                                                    \
    return P##_create_predefined_returning_value_program(pre_def); /* one object serves both kinds */                 \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_generate_program(icicle_symbol_handle_t* parameters, int nof_parameters, icicle_program_handle_t* program)                    \
  {                                                                                                                    \
    SC_GUARDED(program_generate(ScFieldOf<PR>::type::W, parameters, nof_parameters, program, true))                    \
  }                                                                                                                    \
  extern "C" icicle_symbol_handle_t P##_create_input_symbol(int in_idx)                                                \
  {                                                                                                                    \
    try {                                                                                                              \
      return symbol_new(ScFieldOf<PR>::type::W, sym_input(in_idx));                                                    \
    } catch (...) {                                                                                                    \
      return nullptr;                                                                                                  \
    }                                                                                                                  \
  }                                                                                                                    \
  extern "C" icicle_symbol_handle_t P##_create_scalar_symbol(const uint32_t* constant)                                 \
  {                                                                                                                    \
    if (!constant || !ScFieldOf<PR>::type::host_field().is_canonical(constant)) return nullptr;                        \
    try {                                                                                                              \
      return symbol_new(ScFieldOf<PR>::type::W, sym_const(constant, ScFieldOf<PR>::type::W));                          \
    } catch (...) {                                                                                                    \
      return nullptr;                                                                                                  \
    }                                                                                                                  \
  }                                                                                                                    \
  extern "C" icicle_symbol_handle_t P##_copy_symbol(icicle_symbol_handle_t other)                                      \
  {                                                                                                                    \
    if (!other || ((const SymbolObj*)other)->words != ScFieldOf<PR>::type::W) return nullptr;                          \
    try {                                                                                                              \
      return symbol_new(ScFieldOf<PR>::type::W, ((const SymbolObj*)other)->node);                                      \
    } catch (...) {                                                                                                    \
      return nullptr;                                                                                                  \
    }                                                                                                                  \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_add_symbols(icicle_symbol_handle_t op_a, icicle_symbol_handle_t op_b, icicle_symbol_handle_t* res)                            \
  {                                                                                                                    \
    SC_GUARDED(symbol_binary(ScFieldOf<PR>::type::W, PROG_ADD, op_a, op_b, res))                                       \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_sub_symbols(icicle_symbol_handle_t op_a, icicle_symbol_handle_t op_b, icicle_symbol_handle_t* res)                            \
  {                                                                                                                    \
    SC_GUARDED(symbol_binary(ScFieldOf<PR>::type::W, PROG_SUB, op_a, op_b, res))                                       \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_multiply_symbols(icicle_symbol_handle_t op_a, icicle_symbol_handle_t op_b, icicle_symbol_handle_t* res)                       \
  {                                                                                                                    \
    SC_GUARDED(symbol_binary(ScFieldOf<PR>::type::W, PROG_MUL, op_a, op_b, res))                                       \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_inverse_symbol(icicle_symbol_handle_t input, icicle_symbol_handle_t* output)           \
  {                                                                                                                    \
    SC_GUARDED(symbol_inverse(ScFieldOf<PR>::type::W, input, output))                                                  \
  }
DEFINE_SUMCHECK(babybear, babybear_params)
DEFINE_SUMCHECK(koalabear, koalabear_params)
DEFINE_SUMCHECK(bn254, bn254_fr_params)
DEFINE_SUMCHECK(bls12_381, bls12_381_fr_params)
