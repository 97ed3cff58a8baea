// vector_inv / vector_div / vector_sum / vector_product for the eight fields of vecops_arith.hip.
//
// Reference semantics: icicle/src/vec_ops.cpp:9 (vector_product), :40 (vector_sum), :217 (vector_div), :250 (vector_inv); CPU backend
// icicle/backend/cpu/src/field/cpu_vec_ops.cpp:158-201, 386-503. Elements are canonical words in and out. inv and div are element-wise
// over size * batch_size elements with 1 / 0 = 0; sum and product write one element per batch entry, entry k holding its element j
// at k * size + j, or at j * batch_size + k with columns_batch.
//
// Inversion shares one a^(p-2) chain among the 64 * K elements of a tile (Montgomery's trick), one tile per wave: no LDS, no barrier.
// The reductions go lane -> wave (shuffles) -> block (LDS) -> one partial per block, and a second launch folds the partials of each
// batch entry. The powers of R of the Montgomery fields are settled once per tile or per entry (vecops_elem.hpp).
#include "vecops_tile.hpp" // InvTile, k_vec_inv, inv_run, k_vec_reduce, k_vec_reduce_finish, reduce_run

using namespace icicle_hip;

#define DEFINE_VEC_INV(NAME, EL)                                                                                       \
  extern "C" icicle_error_t NAME##_vector_inv(const void* a, uint64_t n, const icicle_vec_ops_config_t* c, void* o) { GUARDED((inv_run<EL, false>(a, nullptr, n, c, o))); } \
  extern "C" icicle_error_t NAME##_vector_div(const void* a, const void* b, uint64_t n, const icicle_vec_ops_config_t* c, void* o) { GUARDED((inv_run<EL, true>(a, b, n, c, o))); } \
  extern "C" icicle_error_t NAME##_vector_sum(const void* a, uint64_t n, const icicle_vec_ops_config_t* c, void* o) { GUARDED((reduce_run<EL, RED_SUM>(a, n, c, o))); } \
  extern "C" icicle_error_t NAME##_vector_product(const void* a, uint64_t n, const icicle_vec_ops_config_t* c, void* o) { GUARDED((reduce_run<EL, RED_PRODUCT>(a, n, c, o))); }

DEFINE_VEC_INV(babybear, SmallElem<babybear_params>)
DEFINE_VEC_INV(koalabear, SmallElem<koalabear_params>)
DEFINE_VEC_INV(bn254, BigElem<bn254_fr_params>)
DEFINE_VEC_INV(bls12_381, BigElem<bls12_381_fr_params>)
DEFINE_VEC_INV(bls12_377, BigElem<bls12_377_fr_params>)
DEFINE_VEC_INV(grumpkin, BigElem<bn254_fq_params>)
DEFINE_VEC_INV(stark252, BigElem<stark252_fr_params>)
DEFINE_VEC_INV(goldilocks, GoldElem)

extern "C" int icicle_hip_vector_inv_tile(int words_per_element)
{
  switch (words_per_element) {
  case 1: return 64 * InvTile<SmallElem<babybear_params>>::K;
  case 2: return 64 * InvTile<GoldElem>::K;
  case 8: return 64 * InvTile<BigElem<bn254_fr_params>>::K;
  default: return 0;
  }
}
