// Poseidon2 batch hashing over the scalar fields of BN254, BLS12-381, BLS12-377 and Grumpkin and over stark252 on the device: the
// kernels over poseidon2_wide.hpp and the hasher's state. hash.hip dispatches to the two launchers below from icicle_hasher_hash
// and from every Merkle tree path.
//
// One lane hashes one message, 256 lanes per block, as poseidon2.hip and poseidon.hip. A permutation of width 3 over BN254 is
// 8 * 3 + 56 S-boxes of three products each and no product in either linear layer, 240 Montgomery products for 64 or 96 bytes
// read: the work is far on the compute side of the roof and the lanes' strided loads do not matter. The state of width 8 is 72
// registers and no kernel carries scratch (tests/test_poseidon2_wide_isa.py; profiles/poseidon2_notes.md has the register counts
// and the measured rates). The constants are read through a pointer that is the same for every lane, so they arrive by scalar loads.
#include "common.h"
#include "poseidon2_wide.hpp"
#include "poseidon2_wide_params.h"
#include <algorithm>

namespace icicle_hip {

  template <class PR, int T>
  __global__ __launch_bounds__(256) void k_poseidon2_wide_batch(const uint8_t* __restrict__ in, uint64_t elems, uint64_t stride, uint64_t n, const Poseidon2WideCtx c,
                                                                 uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
      uint32_t d[8];
      Poseidon2Wide<PR, T>::hash(PoseidonWords{reinterpret_cast<const uint32_t*>(in + i * stride)}, elems, c, d);
#pragma unroll
      for (int k = 0; k < 8; k++)
        reinterpret_cast<uint32_t*>(out)[8 * i + k] = d[k];
    }
  }

  template <class PR, int T>
  __global__ __launch_bounds__(256) void k_poseidon2_wide_leaves(const uint8_t* __restrict__ leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid,
                                                                  const uint8_t* __restrict__ last, uint64_t es, const Poseidon2WideCtx c, uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
      uint32_t d[8];
      Poseidon2Wide<PR, T>::hash(PoseidonPadded{ReadPadded{leaves, (first + i) * chunk, valid, last, es}}, chunk / 32, c, d);
#pragma unroll
      for (int k = 0; k < 8; k++)
        reinterpret_cast<uint32_t*>(out)[8 * i + k] = d[k];
    }
  }

  // the constants of one (field, t): derived once per process, uploaded once per device, shared by every hasher of that pair
  struct Poseidon2WideTables {
    int half_f = 0, r_p = 0;
    std::vector<uint32_t> consts; // poseidon2_wide_device_constants
    std::mutex mtx;
    std::vector<std::pair<int, uint32_t*>> on_device; // (device, copy of consts); kept until the process ends, as the constants themselves are
    // the constants on the calling thread's device; the first call per device uploads them, synchronously, so that every stream sees them
    icicle_error_t device_copy(const uint32_t** out)
    {
      int dev = 0;
      HIP_TRY(hipGetDevice(&dev), ICICLE_INVALID_DEVICE);
      std::lock_guard<std::mutex> lk(mtx);
      for (auto& d : on_device)
        if (d.first == dev) {
          *out = d.second;
          return ICICLE_SUCCESS;
        }
      uint32_t* buf = nullptr;
      HIP_TRY(hipMalloc((void**)&buf, 4 * consts.size()), ICICLE_ALLOCATION_FAILED);
      if (hipMemcpy(buf, consts.data(), 4 * consts.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(buf);
        return ICICLE_COPY_FAILED;
      }
      on_device.emplace_back(dev, buf);
      *out = buf;
      return ICICLE_SUCCESS;
    }
  };

  struct Poseidon2WideHasher {
    int field = 0;
    unsigned t = 0;
    bool has_tag = false;
    uint32_t tag[POSEIDON2_WIDE_LIMBS] = {0}; // Montgomery
    Poseidon2WideTables* tables = nullptr;
    icicle_error_t context(Poseidon2WideCtx* c)
    {
      c->half_f = tables->half_f, c->r_p = tables->r_p, c->has_tag = has_tag ? 1u : 0u;
      std::copy(tag, tag + POSEIDON2_WIDE_LIMBS, c->tag);
      return tables->device_copy(&c->consts);
    }
  };

  // nullptr where the derived parameters are not what the lane code is compiled for: its S-box, an even R_F, and at t = 2, 3 the
  // diagonal (2, 3), (2, 2, 3) that M_I applies by additions
  template <class PR>
  static Poseidon2WideTables* poseidon2_wide_tables(unsigned t)
  {
    static std::mutex mtx;
    static Poseidon2WideTables* slots[9] = {nullptr};
    const std::shared_ptr<const poseidon2_wide::Params<PR>> P = poseidon2_wide::params<PR>(t);
    if (!P || P->alpha != poseidon2_wide_alpha<PR>() || P->r_f % 2 != 0) return nullptr;
    if (t < 4) {
      using H = poseidon::HostField<PR>;
      for (unsigned i = 0; i < t; i++)
        if (!poseidon2_wide::fe_equal<PR>(P->diag[i], H::from_small(i + 1 == t ? 3 : 2))) return nullptr;
    }
    std::lock_guard<std::mutex> lk(mtx);
    if (!slots[t]) {
      slots[t] = new Poseidon2WideTables;
      slots[t]->half_f = P->r_f / 2, slots[t]->r_p = P->r_p;
      slots[t]->consts = poseidon2_wide_device_constants<PR>(P->rc, P->diag);
    }
    return slots[t];
  }

  template <class PR>
  static std::shared_ptr<Poseidon2WideHasher> poseidon2_wide_make_field(int field, unsigned t, const uint32_t* tag)
  {
    if (tag && !poseidon::HostField<PR>::below_p(tag)) return nullptr;
    Poseidon2WideTables* tables = poseidon2_wide_tables<PR>(t);
    if (!tables) return nullptr;
    auto h = std::make_shared<Poseidon2WideHasher>();
    h->field = field, h->t = t, h->tables = tables, h->has_tag = tag != nullptr;
    if (tag) {
      const Fe<PR> m = FieldOps<PR>::reduce(FieldOps<PR>::from_canonical(tag));
      std::copy(m.l, m.l + POSEIDON2_WIDE_LIMBS, h->tag);
    }
    return h;
  }

  std::shared_ptr<Poseidon2WideHasher> poseidon2_wide_make(int field, unsigned t, const uint32_t* tag)
  {
    if (!poseidon2_wide::width_supported(t)) return nullptr;
    switch (field) {
    case 0: return poseidon2_wide_make_field<bn254_fr_params>(field, t, tag);
    case 1: return poseidon2_wide_make_field<bls12_381_fr_params>(field, t, tag);
    case 2: return poseidon2_wide_make_field<bls12_377_fr_params>(field, t, tag);
    case 3: return poseidon2_wide_make_field<bn254_fq_params>(field, t, tag); // Grumpkin's scalars are BN254's base field
    case 4: return poseidon2_wide_make_field<stark252_fr_params>(field, t, tag);
    }
    return nullptr;
  }

  static unsigned poseidon2_wide_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 22); }

// one case per (field, width)
#define POSEIDON2_WIDE_WIDTHS(X, F, PR) X(F, PR, 2) X(F, PR, 3) X(F, PR, 4) X(F, PR, 8)
#define POSEIDON2_WIDE_PAIRS(X)                                                                                        \
  POSEIDON2_WIDE_WIDTHS(X, 0, bn254_fr_params)                                                                         \
  POSEIDON2_WIDE_WIDTHS(X, 1, bls12_381_fr_params)                                                                     \
  POSEIDON2_WIDE_WIDTHS(X, 2, bls12_377_fr_params)                                                                     \
  POSEIDON2_WIDE_WIDTHS(X, 3, bn254_fq_params) POSEIDON2_WIDE_WIDTHS(X, 4, stark252_fr_params)

  icicle_error_t poseidon2_wide_launch_batch(Poseidon2WideHasher& h, const uint8_t* in, uint64_t len, uint64_t stride, uint64_t n, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (len == 0 || (len & 31) || (stride & 3) || ((uintptr_t)in & 3) || ((uintptr_t)out & 3)) return ICICLE_INVALID_ARGUMENT;
    Poseidon2WideCtx c;
    ICICLE_TRY(h.context(&c));
    const unsigned grid = poseidon2_wide_grid(n);
    bool launched = false;
#define POSEIDON2_WIDE_CASE(F, PR, T)                                                                                  \
  if (h.field == F && h.t == T) k_poseidon2_wide_batch<PR, T><<<grid, 256, 0, st>>>(in, len / 32, stride, n, c, out), launched = true;
    POSEIDON2_WIDE_PAIRS(POSEIDON2_WIDE_CASE)
#undef POSEIDON2_WIDE_CASE
    if (!launched) return ICICLE_INVALID_ARGUMENT;
    LAUNCH_CHECK("k_poseidon2_wide_batch", st);
    return ICICLE_SUCCESS;
  }

  icicle_error_t poseidon2_wide_launch_leaves(Poseidon2WideHasher& h, const uint8_t* leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid,
                                              const uint8_t* last, uint64_t es, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (chunk == 0 || (chunk & 31) || ((uintptr_t)out & 3)) return ICICLE_INVALID_ARGUMENT;
    Poseidon2WideCtx c;
    ICICLE_TRY(h.context(&c));
    const unsigned grid = poseidon2_wide_grid(n);
    bool launched = false;
#define POSEIDON2_WIDE_CASE(F, PR, T)                                                                                  \
  if (h.field == F && h.t == T) k_poseidon2_wide_leaves<PR, T><<<grid, 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, c, out), launched = true;
    POSEIDON2_WIDE_PAIRS(POSEIDON2_WIDE_CASE)
#undef POSEIDON2_WIDE_CASE
    if (!launched) return ICICLE_INVALID_ARGUMENT;
    LAUNCH_CHECK("k_poseidon2_wide_leaves", st);
    return ICICLE_SUCCESS;
  }

} // namespace icicle_hip
