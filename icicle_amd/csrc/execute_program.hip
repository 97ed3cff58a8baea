// execute_program over BabyBear, KoalaBear (one word) and the BN254, BLS12-381 scalar fields (eight words): a program -- one of the
// two predefined ones, or a function built from symbols and compiled by <field>_generate_program -- evaluated element by element over
// its parameters' vectors, in one launch (include/icicle/vec_ops.h:404, src/vec_ops.cpp:562-587).
//
// Reference semantics: backend/cpu/src/field/cpu_vec_ops.cpp:635-678 and backend/cpu/include/cpu_program_executor.h; the host-only
// rules -- the instruction order, which parameters are read and written, the slots of the variable file -- are in program_plan.h and
// program_lower.h.
//
// Elements are canonical in memory and in Montgomery form between a load and a store. The predefined programs hold their operands in
// registers and convert only A and E: (aR) b / R - c is canonical, and (eR) t / R is. A user program runs on an interpreter over the
// lowered list: one wave per block, the variable file in LDS with a wave's lanes on consecutive words, the list and the constants read
// from device memory at wave-uniform addresses; the block's LDS is sized by the slots the program uses. The loops are grid-stride:
// a lane handles one element per pass (four per 16-byte load or per interpreted instruction for the one-word fields).
#include "program_device.hpp"
#include <cstring>
#include <vector>

namespace icicle_hip {

  constexpr int EP_BLOCK = 256;       // lanes of a block of the predefined kernels
  constexpr int EP_INTERP_BLOCK = 64; // one wave: a lane's variables are a column of the block's LDS
  constexpr unsigned EP_MAX_GRID = 2048;        // blocks of a predefined kernel: 32 waves on each of 256 CUs
  constexpr unsigned EP_INTERP_MAX_GRID = 4096; // blocks of the interpreter: 16 waves per CU where the variable file lets them in

  static_assert(ScSmall<babybear_params>::MONT_BITS == 32 && ScBig<bn254_fr_params>::MONT_BITS == 261 && ScBig<bls12_381_fr_params>::MONT_BITS == 261,
                "tests/execute_program_host_harness.cpp lowers with these");

  struct EpPredefArgs {
    const uint32_t* in[4]; // A, B, C and, for E (A B - C), E
    uint32_t* out;         // may be one of `in`
  };

  template <class FA, int PROG>
  SC_D typename FA::elem ep_predef(const typename FA::elem& a, const typename FA::elem& b, const typename FA::elem& c, const typename FA::elem& e)
  {
    const typename FA::elem t = FA::sub(FA::mul(FA::mul(a, FA::r2()), b), c);
    if constexpr (PROG == PROG_AB_MINUS_C)
      return t;
    else
      return FA::mul(FA::mul(e, FA::r2()), t);
  }

  // element i of a vector whose address is only element-aligned, word by word
  template <class FA>
  SC_D typename FA::elem ep_load(const uint32_t* v, uint64_t i)
  {
    uint32_t w[FA::W];
#pragma unroll
    for (int k = 0; k < FA::W; k++)
      w[k] = v[i * FA::W + k];
    return FA::load(w);
  }
  template <class FA>
  SC_D void ep_store(uint32_t* v, uint64_t i, const typename FA::elem& e)
  {
    uint32_t w[FA::W];
    FA::store(w, e);
#pragma unroll
    for (int k = 0; k < FA::W; k++)
      v[i * FA::W + k] = w[k];
  }

  // VEC = 4 (one-word fields, every pointer 16-byte aligned): four elements per 16-byte load, the n % 4 last ones by the first lanes.
  // VEC = 1: one element per lane and pass, at any element-aligned address.
  template <class PR, int PROG, int VEC>
  __global__ __launch_bounds__(EP_BLOCK) void k_execute_predef(EpPredefArgs p, uint64_t n)
  {
    using FA = typename ScFieldOf<PR>::type;
    using elem = typename FA::elem;
    constexpr int M = PROG == PROG_AB_MINUS_C ? 3 : 4;
    const uint64_t stride = (uint64_t)gridDim.x * EP_BLOCK, first = (uint64_t)blockIdx.x * EP_BLOCK + threadIdx.x;
    uint64_t begin = first;
    if constexpr (VEC == 4) {
      static_assert(FA::W == 1, "wide loads are for the one-word fields");
      const uint64_t quads = n / 4;
      for (uint64_t t = first; t < quads; t += stride) {
        uint4 v[4];
#pragma unroll
        for (int j = 0; j < M; j++)
          v[j] = reinterpret_cast<const uint4*>(p.in[j])[t];
        if constexpr (M == 3) v[3] = make_uint4(0, 0, 0, 0);
        uint4 o;
        o.x = ep_predef<FA, PROG>(v[0].x, v[1].x, v[2].x, v[3].x);
        o.y = ep_predef<FA, PROG>(v[0].y, v[1].y, v[2].y, v[3].y);
        o.z = ep_predef<FA, PROG>(v[0].z, v[1].z, v[2].z, v[3].z);
        o.w = ep_predef<FA, PROG>(v[0].w, v[1].w, v[2].w, v[3].w);
        reinterpret_cast<uint4*>(p.out)[t] = o;
      }
      begin = 4 * quads + first;
    }
    for (uint64_t i = begin; i < n; i += stride) {
      elem x[4];
#pragma unroll
      for (int j = 0; j < M; j++)
        x[j] = ep_load<FA>(p.in[j], i);
      if constexpr (M == 3) x[3] = FA::zero();
      ep_store<FA>(p.out, i, ep_predef<FA, PROG>(x[0], x[1], x[2], x[3]));
    }
  }

  // ---- user programs: an interpreter over the lowered list -------------------------------------------------------------------------
  struct EpPtrs {
    uint32_t* p[256]; // by parameter; only those the list loads or stores are read
  };

  // A lane works on E elements at once, so that the E chains of loads, LDS accesses and multiplications overlap and one fetch of an
  // instruction serves them all: 4 for the one-word fields, 1 for the eight-word ones, whose file is 9 words per value. Word q of
  // copy e of slot s of lane l at [((s E + e) REGS + q) 64 + l] (per copy the layout of sumcheck.hip's ScVars).
  template <class FA>
  struct EpVars {
    static constexpr int SLOTS = FA::W == 1 ? EP_CAP_SMALL : EP_CAP_BIG, E = FA::W == 1 ? 4 : 1;
    uint32_t* base;
    SC_D typename FA::elem ld(uint32_t slot, int e) const
    {
      typename FA::elem x;
#pragma unroll
      for (int q = 0; q < FA::REGS; q++)
        FA::reg(x, q) = base[((slot * E + e) * FA::REGS + q) * EP_INTERP_BLOCK];
      return x;
    }
    SC_D void st(uint32_t slot, int e, typename FA::elem x) const
    {
#pragma unroll
      for (int q = 0; q < FA::REGS; q++)
        base[((slot * E + e) * FA::REGS + q) * EP_INTERP_BLOCK] = FA::reg(x, q);
    }
  };

  // code: nof_ins words op | a << 8 | b << 16 | dst << 24 over slots below the program's nof_slots <= EpVars::SLOTS (program_lower.h),
  // then nof_constants constants of REGS words each, which go to slots 0 .. nof_constants - 1. Dynamic LDS: nof_slots slots of E
  // copies. A block takes 64 E consecutive elements per pass, lane l the elements l, 64 + l, ..: every access of a wave is contiguous.
  template <class PR>
  __global__ __launch_bounds__(EP_INTERP_BLOCK) void k_execute_program(EpPtrs ptrs, const uint32_t* __restrict__ code, int nof_ins, int nof_constants, uint64_t n)
  {
    using FA = typename ScFieldOf<PR>::type;
    using elem = typename FA::elem;
    constexpr int E = EpVars<FA>::E;
    extern __shared__ uint32_t ep_file[]; // the slots the program uses (the launch sizes it), at most EpVars::SLOTS
    const EpVars<FA> v{ep_file + threadIdx.x};
    const uint32_t* constants = code + nof_ins;
    for (int c = 0; c < nof_constants; c++) {
      elem x = FA::zero();
#pragma unroll
      for (int q = 0; q < FA::REGS; q++)
        FA::reg(x, q) = constants[c * FA::REGS + q];
#pragma unroll
      for (int e = 0; e < E; e++)
        v.st(c, e, x);
    }
    const uint64_t chunks = (n + EP_INTERP_BLOCK * E - 1) / (EP_INTERP_BLOCK * E);
    for (uint64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
      const uint64_t i0 = chunk * (EP_INTERP_BLOCK * E) + threadIdx.x; // copy e: element i0 + 64 e, idle past the end
      for (int q = 0; q < nof_ins; q++) {
        const uint32_t ins = code[q];
        const uint32_t op = ins & 0xff, ia = (ins >> 8) & 0xff, ib = (ins >> 16) & 0xff, id = ins >> 24;
        if (op == EP_LOAD) {
          const uint32_t* src = ptrs.p[ia];
          elem x[E];
#pragma unroll
          for (int e = 0; e < E; e++)
            x[e] = i0 + EP_INTERP_BLOCK * e < n ? ep_load<FA>(src, i0 + EP_INTERP_BLOCK * e) : FA::zero();
#pragma unroll
          for (int e = 0; e < E; e++)
            v.st(id, e, FA::mul(x[e], FA::r2()));
        } else if (op == EP_STORE) {
          uint32_t* dst = ptrs.p[ib];
#pragma unroll
          for (int e = 0; e < E; e++)
            if (i0 + EP_INTERP_BLOCK * e < n) ep_store<FA>(dst, i0 + EP_INTERP_BLOCK * e, FA::mul(v.ld(ia, e), FA::plain_one()));
        } else {
          elem a[E], r[E];
#pragma unroll
          for (int e = 0; e < E; e++)
            r[e] = a[e] = v.ld(ia, e); // PROG_COPY
          if (op == PROG_INV) {
#pragma unroll
            for (int e = 0; e < E; e++)
              r[e] = FA::inv(a[e]);
          } else if (op != PROG_COPY) {
            elem b[E];
#pragma unroll
            for (int e = 0; e < E; e++)
              b[e] = v.ld(ib, e);
#pragma unroll
            for (int e = 0; e < E; e++)
              r[e] = op == PROG_MUL ? FA::mul(a[e], b[e]) : op == PROG_ADD ? FA::add(a[e], b[e]) : FA::sub(a[e], b[e]);
          }
#pragma unroll
          for (int e = 0; e < E; e++)
            v.st(id, e, r[e]);
        }
      }
    }
  }

  // ---- the host side -----------------------------------------------------------------------------------------------------------------
  // the lowered program of `obj` (made on the first call), 0 when it can run
  template <class FA>
  static int lowered_of(ProgramObj* obj)
  {
    std::lock_guard<std::mutex> lk(obj->mtx);
    if (obj->lower_state < 0) obj->lower_state = program_lower(FA::host_field(), FA::MONT_BITS, obj->prog, program_live_cap(FA::W), &obj->lowered);
    return obj->lower_state;
  }

  // the list and the constants in the current device's memory, uploaded once per program and device
  template <class FA>
  static icicle_error_t device_code_of(ProgramObj* obj, const uint32_t** d_code)
  {
    std::lock_guard<std::mutex> lk(obj->mtx);
    const int dev = current_device_id();
    if (obj->d_code && obj->d_device == dev) {
      *d_code = (const uint32_t*)obj->d_code;
      return ICICLE_SUCCESS;
    }
    const LoweredProgram& l = obj->lowered;
    std::vector<uint32_t> h(l.code);
    for (const auto& c : l.constants) {
      typename FA::elem e = FA::load(c.data());
      for (int q = 0; q < FA::REGS; q++)
        h.push_back(FA::reg(e, q));
    }
    if (obj->d_code) {
      (void)hipFree(obj->d_code);
      obj->d_code = nullptr;
    }
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, h.size() * 4 + 16), ICICLE_ALLOCATION_FAILED);
    if (hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(d);
      return ICICLE_COPY_FAILED;
    }
    obj->d_code = d, obj->d_device = dev;
    *d_code = (const uint32_t*)d;
    return ICICLE_SUCCESS;
  }

  template <class PR, int PROG>
  static void launch_predef(const EpPredefArgs& a, uint64_t n, hipStream_t st)
  {
    using FA = typename ScFieldOf<PR>::type;
    constexpr int M = PROG == PROG_AB_MINUS_C ? 3 : 4;
    bool wide = FA::W == 1 && ((uintptr_t)a.out & 15) == 0;
    for (int j = 0; j < M; j++)
      wide = wide && ((uintptr_t)a.in[j] & 15) == 0;
    const uint64_t items = wide ? std::max<uint64_t>(n / 4, 1) : n;
    const unsigned grid = (unsigned)std::min<uint64_t>((items + EP_BLOCK - 1) / EP_BLOCK, EP_MAX_GRID);
    if constexpr (FA::W == 1) {
      if (wide) {
        k_execute_predef<PR, PROG, 4><<<grid, EP_BLOCK, 0, st>>>(a, n);
        return;
      }
    }
    k_execute_predef<PR, PROG, 1><<<grid, EP_BLOCK, 0, st>>>(a, n);
  }

  template <class PR>
  static icicle_error_t execute_program_run(void** data, uint64_t nof_params, ProgramObj* program, uint64_t size, const icicle_vec_ops_config_t* cfg)
  {
    using FA = typename ScFieldOf<PR>::type;
    constexpr size_t EB = 4 * FA::W;
    if (!program || !data || !cfg) return ICICLE_INVALID_POINTER;
    if (nof_params != (uint64_t)program->prog.nof_parameters) return ICICLE_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < nof_params; i++)
      if (!data[i]) return ICICLE_INVALID_POINTER;
    if (program->words != FA::W) return ICICLE_INVALID_ARGUMENT;
    if (lowered_of<FA>(program) != 0) return ICICLE_INVALID_ARGUMENT; // over the cap on live values, or no program of the compiler's
    const uint64_t batch = cfg->batch_size > 1 ? (uint64_t)cfg->batch_size : 1; // columns_batch changes nothing: element-wise
    if (size > (((uint64_t)1 << 48) / batch)) return ICICLE_INVALID_ARGUMENT;
    const uint64_t n = size * batch;
    if (n == 0) return ICICLE_SUCCESS;
    const LoweredProgram& l = program->lowered;
    const int np = l.nof_parameters;

    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    // host data: one staging vector per distinct pointer among the parameters the program touches
    const bool on_host = !cfg->is_a_on_device;
    const size_t pitch = (size_t)((n * EB + 15) & ~(uint64_t)15);
    TempBuf staging;
    std::vector<uint32_t*> dev(np, nullptr);
    std::vector<int> owner(np, -1); // the first parameter with the same host pointer
    std::vector<uint8_t> use(np, 0); // per owner: the uses of all its parameters
    if (on_host) {
      int count = 0;
      std::vector<int> index(np, -1);
      for (int j = 0; j < np; j++) {
        if (!l.param_use[j]) continue;
        for (int k = 0; k < j && owner[j] < 0; k++)
          if (l.param_use[k] && data[k] == data[j]) owner[j] = owner[k];
        if (owner[j] < 0) owner[j] = j, index[j] = count++;
        use[owner[j]] |= l.param_use[j];
      }
      HIP_TRY(staging.alloc(pitch * (size_t)count, st), ICICLE_ALLOCATION_FAILED);
      for (int j = 0; j < np; j++) {
        if (owner[j] < 0) continue;
        dev[j] = reinterpret_cast<uint32_t*>(staging.as<uint8_t>() + pitch * (size_t)index[owner[j]]);
        if (owner[j] == j && (use[j] & EP_READ)) HIP_TRY(hipMemcpyAsync(dev[j], data[j], n * EB, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
      }
    } else {
      for (int j = 0; j < np; j++)
        dev[j] = (uint32_t*)data[j];
    }

    if (l.predefined >= 0) {
      EpPredefArgs a{};
      for (int j = 0; j + 1 < np; j++)
        a.in[j] = dev[j];
      a.out = dev[np - 1];
      if (l.predefined == PROG_AB_MINUS_C)
        launch_predef<PR, PROG_AB_MINUS_C>(a, n, st);
      else
        launch_predef<PR, PROG_EQ_X_AB_MINUS_C>(a, n, st);
      LAUNCH_CHECK("k_execute_predef", st);
    } else if (!l.code.empty()) {
      const uint32_t* d_code = nullptr;
      ICICLE_TRY(device_code_of<FA>(program, &d_code));
      EpPtrs ptrs{};
      for (int j = 0; j < np; j++)
        ptrs.p[j] = l.param_use[j] ? dev[j] : nullptr;
      constexpr int PER_BLOCK = EP_INTERP_BLOCK * EpVars<FA>::E; // elements of a block and pass
      const unsigned grid = (unsigned)std::min<uint64_t>((n + PER_BLOCK - 1) / PER_BLOCK, EP_INTERP_MAX_GRID);
      static_assert(EpVars<FA>::SLOTS * FA::REGS * PER_BLOCK * 4 <= 64 * 1024, "the variable file of a block");
      const size_t lds = (size_t)std::max(l.nof_slots, 1) * FA::REGS * PER_BLOCK * sizeof(uint32_t);
      k_execute_program<PR><<<grid, EP_INTERP_BLOCK, lds, st>>>(ptrs, d_code, (int)l.code.size(), l.nof_constants, n);
      LAUNCH_CHECK("k_execute_program", st);
    }

    if (on_host) {
      for (int j = 0; j < np; j++)
        if (owner[j] == j && (use[j] & EP_WRITTEN)) HIP_TRY(hipMemcpyAsync(data[j], dev[j], n * EB, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
      HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    } else if (!cfg->is_async) {
      HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    }
    return ICICLE_SUCCESS;
  }

} // namespace icicle_hip

using namespace icicle_hip;

#define DEFINE_EXECUTE_PROGRAM(P, PR)                                                                                  \
  extern "C" icicle_error_t P##_execute_program(void** data, uint64_t nof_params, icicle_program_handle_t program, uint64_t size, const icicle_vec_ops_config_t* config) \
  {                                                                                                                    \
    try {                                                                                                              \
      return execute_program_run<PR>(data, nof_params, (ProgramObj*)program, size, config);                            \
    } catch (...) {                                                                                                    \
      return ICICLE_ALLOCATION_FAILED;                                                                                 \
    }                                                                                                                  \
  }
DEFINE_EXECUTE_PROGRAM(babybear, babybear_params)
DEFINE_EXECUTE_PROGRAM(koalabear, koalabear_params)
DEFINE_EXECUTE_PROGRAM(bn254, bn254_fr_params)
DEFINE_EXECUTE_PROGRAM(bls12_381, bls12_381_fr_params)
