// Poseidon batch hashing over the scalar fields of BN254, BLS12-381, BLS12-377 and Grumpkin on the device: the kernels over
// poseidon.hpp and the hasher's state. hash.hip dispatches to the two launchers below from icicle_hasher_hash and from every Merkle
// tree path.
//
// One lane hashes one message, at every width. A hash of width 3 is 590 products of 81 multiply-adds plus 434 Montgomery
// reductions of 81 more, for 64 or 96 bytes read; width 12 is 2803 products and 1383 reductions for 352 or 384 bytes: the work is
// far on the compute side of the roof and the lanes' strided loads do not matter. What matters is where the state lives. At
// widths 3 and 5 it is 27 and 45 registers and the kernels carry no scratch (tests/test_poseidon_isa.py). At widths 9 and 12 the
// state is 81 and 108 registers and a matrix product needs the old and the new state at once; a block of 256 lanes is one wave
// per SIMD, which may use the whole register file of 512 registers per lane, so the state still has a place in registers, at an
// occupancy of one wave and without scratch (profiles/poseidon_notes.md has the numbers and what a lane group would have to
// exchange instead).
#include "common.h"
#include "poseidon.hpp"
#include "poseidon_params.h"
#include <algorithm>

namespace icicle_hip {

  template <class PR, int T>
  __global__ __launch_bounds__(256) void k_poseidon_batch(const uint8_t* __restrict__ in, uint64_t stride, uint64_t n, const PoseidonCtx c, uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
      uint32_t d[8];
      Poseidon<PR, T>::hash(PoseidonWords{reinterpret_cast<const uint32_t*>(in + i * stride)}, c, d);
#pragma unroll
      for (int k = 0; k < 8; k++)
        reinterpret_cast<uint32_t*>(out)[8 * i + k] = d[k];
    }
  }

  template <class PR, int T>
  __global__ __launch_bounds__(256) void k_poseidon_leaves(const uint8_t* __restrict__ leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid,
                                                            const uint8_t* __restrict__ last, uint64_t es, const PoseidonCtx c, uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
      uint32_t d[8];
      Poseidon<PR, T>::hash(PoseidonPadded{ReadPadded{leaves, (first + i) * chunk, valid, last, es}}, c, d);
#pragma unroll
      for (int k = 0; k < 8; k++)
        reinterpret_cast<uint32_t*>(out)[8 * i + k] = d[k];
    }
  }

  // the tables of one (field, t): derived once per process, uploaded once per device, shared by every hasher of that pair
  struct PoseidonTables {
    int r_p = 0;
    std::vector<uint32_t> tab; // poseidon_device_tables
    std::mutex mtx;
    std::vector<std::pair<int, uint32_t*>> on_device; // (device, copy of tab); kept until the process ends, as the tables themselves are
    // the tables on the calling thread's device; the first call per device uploads them, synchronously, so that every stream sees them
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
      HIP_TRY(hipMalloc((void**)&buf, 4 * tab.size()), ICICLE_ALLOCATION_FAILED);
      if (hipMemcpy(buf, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(buf);
        return ICICLE_COPY_FAILED;
      }
      on_device.emplace_back(dev, buf);
      *out = buf;
      return ICICLE_SUCCESS;
    }
  };

  struct PoseidonHasher {
    int field = 0;
    unsigned t = 0;
    bool has_tag = false;
    uint32_t tag[POSEIDON_LIMBS] = {0}; // Montgomery
    PoseidonTables* tables = nullptr;
    icicle_error_t context(PoseidonCtx* c)
    {
      c->r_p = tables->r_p, c->has_tag = has_tag ? 1u : 0u;
      std::copy(tag, tag + POSEIDON_LIMBS, c->tag);
      return tables->device_copy(&c->tab);
    }
  };

  template <class PR>
  static PoseidonTables* poseidon_tables(unsigned t)
  {
    static std::mutex mtx;
    static PoseidonTables* slots[13] = {nullptr};
    const std::shared_ptr<const poseidon::Params<PR>> P = poseidon::params<PR>(t);
    if (!P) return nullptr;
    std::lock_guard<std::mutex> lk(mtx);
    if (!slots[t]) {
      slots[t] = new PoseidonTables;
      slots[t]->r_p = P->r_p;
      slots[t]->tab = poseidon_device_tables<Fe<PR>>((int)t, P->rc, P->mds, P->pre, P->sparse);
    }
    return slots[t];
  }

  template <class PR>
  static std::shared_ptr<PoseidonHasher> poseidon_make_field(int field, unsigned t, const uint32_t* tag)
  {
    if (tag && !poseidon::HostField<PR>::below_p(tag)) return nullptr;
    PoseidonTables* tables = poseidon_tables<PR>(t);
    if (!tables) return nullptr;
    auto h = std::make_shared<PoseidonHasher>();
    h->field = field, h->t = t, h->tables = tables, h->has_tag = tag != nullptr;
    if (tag) {
      const Fe<PR> m = FieldOps<PR>::reduce(FieldOps<PR>::from_canonical(tag));
      std::copy(m.l, m.l + POSEIDON_LIMBS, h->tag);
    }
    return h;
  }

  std::shared_ptr<PoseidonHasher> poseidon_make(int field, unsigned t, const uint32_t* tag)
  {
    if (!poseidon::width_supported(t)) return nullptr;
    switch (field) {
    case 0: return poseidon_make_field<bn254_fr_params>(field, t, tag);
    case 1: return t == 3 ? nullptr : poseidon_make_field<bls12_381_fr_params>(field, t, tag); // the reference's tables for t = 3 define nothing
    case 2: return poseidon_make_field<bls12_377_fr_params>(field, t, tag);
    case 3: return poseidon_make_field<bn254_fq_params>(field, t, tag); // Grumpkin's scalars are BN254's base field
    }
    return nullptr;
  }

  static unsigned poseidon_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 22); }

// one case per (field, width)
#define POSEIDON_WIDTHS(X, F, PR) X(F, PR, 3) X(F, PR, 5) X(F, PR, 9) X(F, PR, 12)
#define POSEIDON_PAIRS(X)                                                                                              \
  POSEIDON_WIDTHS(X, 0, bn254_fr_params)                                                                               \
  X(1, bls12_381_fr_params, 5) X(1, bls12_381_fr_params, 9) X(1, bls12_381_fr_params, 12)                              \
  POSEIDON_WIDTHS(X, 2, bls12_377_fr_params) POSEIDON_WIDTHS(X, 3, bn254_fq_params)

  icicle_error_t poseidon_launch_batch(PoseidonHasher& h, const uint8_t* in, uint64_t len, uint64_t stride, uint64_t n, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (len != 32ull * (h.t - (h.has_tag ? 1 : 0)) || (stride & 3) || ((uintptr_t)in & 3) || ((uintptr_t)out & 3)) return ICICLE_INVALID_ARGUMENT;
    PoseidonCtx c;
    ICICLE_TRY(h.context(&c));
    const unsigned grid = poseidon_grid(n);
    bool launched = false;
#define POSEIDON_CASE(F, PR, T)                                                                                        \
  if (h.field == F && h.t == T) k_poseidon_batch<PR, T><<<grid, 256, 0, st>>>(in, stride, n, c, out), launched = true;
    POSEIDON_PAIRS(POSEIDON_CASE)
#undef POSEIDON_CASE
    if (!launched) return ICICLE_INVALID_ARGUMENT;
    LAUNCH_CHECK("k_poseidon_batch", st);
    return ICICLE_SUCCESS;
  }

  icicle_error_t poseidon_launch_leaves(PoseidonHasher& h, const uint8_t* leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid, const uint8_t* last,
                                        uint64_t es, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (chunk != 32ull * (h.t - (h.has_tag ? 1 : 0)) || ((uintptr_t)out & 3)) return ICICLE_INVALID_ARGUMENT;
    PoseidonCtx c;
    ICICLE_TRY(h.context(&c));
    const unsigned grid = poseidon_grid(n);
    bool launched = false;
#define POSEIDON_CASE(F, PR, T)                                                                                        \
  if (h.field == F && h.t == T) k_poseidon_leaves<PR, T><<<grid, 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, c, out), launched = true;
    POSEIDON_PAIRS(POSEIDON_CASE)
#undef POSEIDON_CASE
    if (!launched) return ICICLE_INVALID_ARGUMENT;
    LAUNCH_CHECK("k_poseidon_leaves", st);
    return ICICLE_SUCCESS;
  }

} // namespace icicle_hip
