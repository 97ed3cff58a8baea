/*
 * icicle_hip.h -- C ABI of libicicle_hip.so, the MI355X (gfx950) backend for ICICLE's MSM / NTT hot path.
 *
 * Every entry point below has the NAME, ARGUMENT ORDER, STRUCT LAYOUT and ERROR CODES of the
 * extern "C" symbol the reference's Rust / Go wrappers bind (wrappers/rust/icicle-core/src/msm/mod.rs:249-266,
 * ntt/mod.rs:285-293,346-355, icicle-runtime/src/runtime.rs:10-54; wrappers/golang/curves/bn254/msm/include/msm.h:15-16),
 * so those bindings link against this library unchanged. Each declaration cites the reference
 * definition it replaces (paths relative to /root/reference/icicle).
 *
 * Plain C: pointers and sizes only. C++ references in the reference's extern "C" signatures
 * (`const Device&`, `int&`) are passed as pointers here -- the same machine ABI.
 */
#ifndef ICICLE_HIP_H
#define ICICLE_HIP_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
  #include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- errors: include/icicle/errors.h:13-29. Only 0..11 are ever returned (Rust's enum stops at 12). ---- */
typedef enum {
  ICICLE_SUCCESS = 0,
  ICICLE_INVALID_DEVICE = 1,
  ICICLE_OUT_OF_MEMORY = 2,
  ICICLE_INVALID_POINTER = 3,
  ICICLE_ALLOCATION_FAILED = 4,
  ICICLE_DEALLOCATION_FAILED = 5,
  ICICLE_COPY_FAILED = 6,
  ICICLE_SYNCHRONIZATION_FAILED = 7,
  ICICLE_STREAM_CREATION_FAILED = 8,
  ICICLE_STREAM_DESTRUCTION_FAILED = 9,
  ICICLE_API_NOT_IMPLEMENTED = 10,
  ICICLE_INVALID_ARGUMENT = 11
} icicle_error_t;

/* ---- device: include/icicle/device.h:14-48 (sizeof 68, id at offset 64) ---- */
typedef struct {
  char type[64]; /* "HIP" */
  int id;        /* GPU ordinal */
} icicle_device_t;

/* include/icicle/device.h:53-58 */
typedef struct {
  bool using_host_memory;
  int num_memory_regions;
  bool supports_pinned_memory;
} icicle_device_properties_t;

typedef void* icicleStreamHandle; /* a hipStream_t; NULL = default stream (include/icicle/runtime.h) */

/* ======================================================================================
 * Runtime: include/icicle/runtime.h:17-281, src/runtime.cpp.
 * The only registered device type is "HIP". Pointers returned by icicle_malloc* are recorded in an
 * allocation tracker (include/icicle/memory_tracker.h:16-44) so icicle_copy can infer direction.
 * ====================================================================================== */
icicle_error_t icicle_load_backend(const char* path, bool is_recursive); /* runtime.h:17  (no-op: backend is linked in) */
icicle_error_t icicle_load_backend_from_env_or_default(void);            /* runtime.h:29  (no-op) */
icicle_error_t icicle_set_device(const icicle_device_t* device);         /* runtime.h:37 */
icicle_error_t icicle_set_default_device(const icicle_device_t* device); /* runtime.h:45 */
icicle_error_t icicle_get_active_device(icicle_device_t* device);        /* runtime.h:53 */
icicle_error_t icicle_is_host_memory(const void* ptr);                   /* runtime.h:61 */
icicle_error_t icicle_is_active_device_memory(const void* ptr);          /* runtime.h:69 */
icicle_error_t icicle_get_device_count(int* device_count);               /* runtime.h:77 */
icicle_error_t icicle_malloc(void** ptr, size_t size);                   /* runtime.h:86 */
icicle_error_t icicle_malloc_async(void** ptr, size_t size, icicleStreamHandle stream); /* runtime.h:97 */
icicle_error_t icicle_free(void* ptr);                                   /* runtime.h:105 */
icicle_error_t icicle_free_async(void* ptr, icicleStreamHandle stream);  /* runtime.h:114 */
icicle_error_t icicle_get_available_memory(size_t* total, size_t* free); /* runtime.h:123 */
icicle_error_t icicle_memset(void* ptr, int value, size_t size);         /* runtime.h:135 */
icicle_error_t icicle_memset_async(void* ptr, int value, size_t size, icicleStreamHandle stream); /* runtime.h:149 */
icicle_error_t icicle_copy(void* dst, const void* src, size_t size);     /* runtime.h:161 */
icicle_error_t icicle_copy_async(void* dst, const void* src, size_t size, icicleStreamHandle stream); /* :172 */
icicle_error_t icicle_copy_to_host(void* dst, const void* src, size_t size);                          /* :184 */
icicle_error_t icicle_copy_to_host_async(void* dst, const void* src, size_t size, icicleStreamHandle stream); /* :195 */
icicle_error_t icicle_copy_to_device(void* dst, const void* src, size_t size);                        /* :205 */
icicle_error_t icicle_copy_to_device_async(void* dst, const void* src, size_t size, icicleStreamHandle stream); /* :216 */
icicle_error_t icicle_create_stream(icicleStreamHandle* stream);         /* runtime.h:227 */
icicle_error_t icicle_destroy_stream(icicleStreamHandle stream);         /* runtime.h:236 */
icicle_error_t icicle_stream_synchronize(icicleStreamHandle stream);     /* runtime.h:246 */
icicle_error_t icicle_device_synchronize(void);                          /* runtime.h:253 */
icicle_error_t icicle_get_device_properties(icicle_device_properties_t* properties); /* runtime.h:261 */
icicle_error_t icicle_is_device_available(const icicle_device_t* dev);   /* runtime.h:271 */
icicle_error_t icicle_get_registered_devices(char* output, size_t output_size); /* runtime.h:281 */

/* ---- ConfigExtension: src/config_extension.cpp:7-37 (string-keyed int/bool bag, opaque handle) ----
 * The reference hands backend-specific knobs to a backend through MSMConfig.ext / NTTConfig.ext
 * (include/icicle/backend/msm_config.h:4-16, ntt_config.h:9-18). Keys read by this backend:
 *   "hip_num_devices"          (int,  msm + ntt)  G >= 1: run the call on G shards over min(G, visible GPUs) devices
 *                                                 starting at the active one (MSM: contiguous (scalar, base) shards,
 *                                                 partial results all-gathered over RCCL and summed; batched NTT:
 *                                                 rows per device, no collective). icicle_amd/csrc/msm_multi.hpp.
 *   "hip_msm_exchange_buckets" (bool, msm)        with hip_num_devices: exchange bucket slices (all-to-all) instead of
 *                                                 final partial sums, so that the bucket reduction is sharded too.
 * Foreign keys (the CUDA backend's "large_bucket_factor", "fast_twiddles", the CPU backend's "n_threads", ...) are
 * tolerated and ignored. */
typedef struct icicle_config_extension icicle_config_extension_t;
icicle_config_extension_t* create_config_extension(void);
void destroy_config_extension(icicle_config_extension_t* ext);
void config_extension_set_int(icicle_config_extension_t* ext, const char* key, int value);
void config_extension_set_bool(icicle_config_extension_t* ext, const char* key, bool value);
int config_extension_get_int(const icicle_config_extension_t* ext, const char* key);
bool config_extension_get_bool(const icicle_config_extension_t* ext, const char* key);
icicle_config_extension_t* clone_config_extension(const icicle_config_extension_t* ext);

/* ======================================================================================
 * MSM: include/icicle/msm.h:21-53 (MSMConfig, 40 bytes), src/msm.cpp:12-16, 45-49.
 * scalars: batch*N canonical (or reference-Montgomery) scalar_t = 8 x u32 little-endian.
 * bases:   affine_t {x,y}, 2*L x u32 (L = 8 bn254, 12 bls12_381); identity = (0,0).
 * results: batch projective_t {x,y,z}, 3*L x u32, canonical; identity = (0:1:0).
 * ====================================================================================== */
typedef struct {
  icicleStreamHandle stream;       /* offset 0  */
  int precompute_factor;           /* 8  */
  int c;                           /* 12 */
  int bitsize;                     /* 16 */
  int batch_size;                  /* 20 */
  bool are_points_shared_in_batch; /* 24 */
  bool are_scalars_on_device;      /* 25 */
  bool are_scalars_montgomery_form;/* 26 */
  bool are_points_on_device;       /* 27 */
  bool are_points_montgomery_form; /* 28 */
  bool are_results_on_device;      /* 29 */
  bool is_async;                   /* 30 */
  icicle_config_extension_t* ext;  /* 32 */
} icicle_msm_config_t;

/* <curve>_msm_precompute_bases: `nof_bases` is the number of bases of ONE MSM, as both wrappers of the reference pass it
 * (wrappers/rust/icicle-core/src/msm/mod.rs:296, wrappers/golang/curves/bn254/msm/msm.go:39-43): with per-MSM bases
 * (batch_size > 1, are_points_shared_in_batch = false) input_bases holds nof_bases * batch_size points and output_bases
 * takes precompute_factor times as many; layout output[precompute_factor * i + j] = 2^(j * shift) * input[i]
 * (backend/cpu/src/curve/cpu_msm.hpp:470-485). The output is device memory whenever the pointer says so, even with
 * are_results_on_device left false (the Rust wrapper never sets it for this call).
 * Window size with a table: pass the same config.c > 0 to both calls, or leave both at 0 -- then msm() takes the c the table
 * was built with from a per-process record of the tables msm_precompute_bases wrote (any aligned slice of a device-resident
 * table works, a host-resident one is recognised at its start; whatever msm_size / batch_size), and only for a table it has never seen (copied, loaded from disk) derives c from
 * msm_size, scalar bits and precompute_factor exactly as msm_precompute_bases does from nof_bases -- the reference's rule
 * (cpu_msm.hpp:466 vs :207), correct when the two sizes are equal. */
icicle_error_t bn254_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results); /* src/msm.cpp:12 */
icicle_error_t bn254_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases); /* src/msm.cpp:45 */
icicle_error_t bls12_381_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results);
icicle_error_t bls12_381_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases);
/* G2 (the reference's G2_ENABLED build): bases are g2_affine_t = {x.c0, x.c1, y.c0, y.c1} over the base field
 * (curves/params/bn254.h:15-17, fields/complex_extension.h), results g2_projective_t = {x, y, z}. Same MSMConfig. */
icicle_error_t bn254_g2_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results); /* src/msm.cpp:28 */
icicle_error_t bn254_g2_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases); /* src/msm.cpp:61 */
icicle_error_t bls12_381_g2_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results);
icicle_error_t bls12_381_g2_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases);

/* ======================================================================================
 * NTT: include/icicle/ntt.h:23-26 (NTTDir), 37-44 (Ordering), 53-64 (NTTConfig<S>), 92-96
 * (NTTInitDomainConfig); src/ntt.cpp:11-84.  NTTConfig<S> for a 4-byte S is 40 bytes.
 * ====================================================================================== */
typedef enum { ICICLE_NTT_FORWARD = 0, ICICLE_NTT_INVERSE = 1 } icicle_ntt_dir_t;
typedef enum { ICICLE_kNN = 0, ICICLE_kNR = 1, ICICLE_kRN = 2, ICICLE_kRR = 3, ICICLE_kNM = 4, ICICLE_kMN = 5 } icicle_ordering_t;

typedef struct {
  icicleStreamHandle stream;      /* 0  */
  uint32_t coset_gen;             /* 8   canonical field element, 1 = no coset */
  int batch_size;                 /* 12 */
  bool columns_batch;             /* 16 */
  int ordering;                   /* 20  icicle_ordering_t */
  bool are_inputs_on_device;      /* 24 */
  bool are_outputs_on_device;     /* 25 */
  bool is_async;                  /* 26 */
  icicle_config_extension_t* ext; /* 32 */
} icicle_ntt_config_u32_t;

typedef struct {
  icicleStreamHandle stream;      /* 0 */
  bool is_async;                  /* 8 */
  icicle_config_extension_t* ext; /* 16 */
} icicle_ntt_init_domain_config_t;

#define ICICLE_HIP_DECLARE_NTT_U32(F)                                                                                  \
  icicle_error_t F##_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u32_t* config, uint32_t* output); /* src/ntt.cpp:11 */ \
  icicle_error_t F##_ntt_init_domain(const uint32_t* primitive_root, const icicle_ntt_init_domain_config_t* config);  /* src/ntt.cpp:26 */ \
  icicle_error_t F##_ntt_release_domain(void);                                                                          /* src/ntt.cpp:41 */ \
  icicle_error_t F##_get_root_of_unity(uint64_t max_size, uint32_t* rou);                                               /* src/ntt.cpp:55 */ \
  icicle_error_t F##_get_root_of_unity_from_domain(uint64_t logn, uint32_t* rou);                                       /* src/ntt.cpp:75 */ \
  icicle_error_t F##_extension_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u32_t* config, uint32_t* output); /* src/ntt.cpp:90 */

ICICLE_HIP_DECLARE_NTT_U32(babybear)
ICICLE_HIP_DECLARE_NTT_U32(koalabear)

/* NTT over the curves' 256-bit scalar fields: scalar_t = 8 little-endian u32 words, so NTTConfig<scalar_t>
 * is 64 bytes (include/icicle/ntt.h:53-64 with S = bn254::scalar_t; storage<8> is 8-byte aligned on the host,
 * include/icicle/math/storage.h:36-49). Symbols: src/ntt.cpp:11-84 built with FIELD = the curve's scalar field. */
typedef struct {
  icicleStreamHandle stream;
  uint32_t coset_gen[8]; /* canonical, {1,0,..} = no coset */
  int32_t batch_size;
  bool columns_batch;
  int32_t ordering; /* icicle_ntt_ordering_t */
  bool are_inputs_on_device;
  bool are_outputs_on_device;
  bool is_async;
  icicle_config_extension_t* ext;
} icicle_ntt_config_u256_t;

#define ICICLE_HIP_DECLARE_NTT_U256(F)                                                                                 \
  icicle_error_t F##_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u256_t* config, uint32_t* output); /* src/ntt.cpp:11 */ \
  icicle_error_t F##_ntt_init_domain(const uint32_t* primitive_root, const icicle_ntt_init_domain_config_t* config);  /* src/ntt.cpp:26 */ \
  icicle_error_t F##_ntt_release_domain(void);                                                                          /* src/ntt.cpp:41 */ \
  icicle_error_t F##_get_root_of_unity(uint64_t max_size, uint32_t* rou);                                               /* src/ntt.cpp:55 */ \
  icicle_error_t F##_get_root_of_unity_from_domain(uint64_t logn, uint32_t* rou);                                       /* src/ntt.cpp:75 */

ICICLE_HIP_DECLARE_NTT_U256(bn254)
ICICLE_HIP_DECLARE_NTT_U256(bls12_381)
/* ECNTT: NTT over G1 points with scalar-field twiddles (src/ecntt.cpp:7-11). input/output: projective_t[size*batch]
 * (3 base-field elements each); config and twiddle domain are those of <curve>_ntt. */
icicle_error_t bn254_ecntt(const void* input, int size, int dir, const icicle_ntt_config_u256_t* config, void* output);
icicle_error_t bls12_381_ecntt(const void* input, int size, int dir, const icicle_ntt_config_u256_t* config, void* output);

/* ======================================================================================
 * Montgomery-form conversion (vec-ops): include/icicle/vec_ops.h:19-37 (VecOpsConfig, 32 bytes),
 * src/vec_ops.cpp:404-408,421-425 (<prefix>_scalar_convert_montgomery, _extension_scalar_convert_montgomery),
 * src/curves/montgomery_conversion.cpp:12-16,46-50 (<curve>_affine/_projective_convert_montgomery).
 * x -> x*R (is_to_montgomery) or x*R^-1 mod p, R = 2^(32*limbs); element-wise, any layout.
 * ====================================================================================== */
typedef struct {
  icicleStreamHandle stream;      /* 0  */
  bool is_a_on_device;            /* 8  */
  bool is_b_on_device;            /* 9  */
  bool is_result_on_device;       /* 10 */
  bool is_async;                  /* 11 */
  int batch_size;                 /* 12 */
  bool columns_batch;             /* 16 */
  icicle_config_extension_t* ext; /* 24 */
} icicle_vec_ops_config_t;

#define ICICLE_HIP_DECLARE_CONVERT(P)                                                                                  \
  icicle_error_t P##_scalar_convert_montgomery(const void* input, uint64_t size, bool is_to_montgomery, const icicle_vec_ops_config_t* config, void* output);
ICICLE_HIP_DECLARE_CONVERT(bn254)
ICICLE_HIP_DECLARE_CONVERT(bls12_381)
ICICLE_HIP_DECLARE_CONVERT(babybear)
ICICLE_HIP_DECLARE_CONVERT(koalabear)
icicle_error_t babybear_extension_scalar_convert_montgomery(const void* input, uint64_t size, bool is_to_montgomery, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t koalabear_extension_scalar_convert_montgomery(const void* input, uint64_t size, bool is_to_montgomery, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t bn254_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t bn254_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t bls12_381_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t bls12_381_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t bn254_g2_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output); /* src/curves/montgomery_conversion.cpp:29 */
icicle_error_t bn254_g2_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output); /* :63 */
icicle_error_t bls12_381_g2_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t bls12_381_g2_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);

/* Element-wise vector operations next to the NTT path, for every NTT field (src/vec_ops.cpp:71-84 vector_add,
 * :136-149 vector_sub, :169-182 vector_mul, :362-366 scalar_mul_vec -- one scalar per batch entry --, :440-444
 * bit_reverse). `size` is per batch entry; config.batch_size / columns_batch as in the reference. */
#define ICICLE_HIP_DECLARE_VEC_ARITH(F)                                                                                \
  icicle_error_t F##_vector_add(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_vector_sub(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_vector_mul(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_scalar_mul_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_scalar_add_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_scalar_sub_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t icicle_hip_##F##_scalar_add_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t icicle_hip_##F##_scalar_sub_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_bit_reverse(const void* input, uint64_t size, const icicle_vec_ops_config_t* config, void* output); \
  icicle_error_t icicle_hip_##F##_vector_add(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t icicle_hip_##F##_vector_sub(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t icicle_hip_##F##_vector_mul(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t icicle_hip_##F##_scalar_mul_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t icicle_hip_##F##_bit_reverse(const void* input, uint64_t size, const icicle_vec_ops_config_t* config, void* output);
ICICLE_HIP_DECLARE_VEC_ARITH(babybear)
ICICLE_HIP_DECLARE_VEC_ARITH(koalabear)
ICICLE_HIP_DECLARE_VEC_ARITH(bn254)
ICICLE_HIP_DECLARE_VEC_ARITH(bls12_381)

/* Inversion, division, sum and product of field vectors, for the fields above and the ones declared with them further down
 * (src/vec_ops.cpp:250 vector_inv, :217 vector_div, :40 vector_sum, :9 vector_product; CPU backend
 * backend/cpu/src/field/cpu_vec_ops.cpp:158-201, 386-503). Elements are canonical words in and out; `size` is per batch entry.
 *  - vector_inv / vector_div are element-wise over size * batch_size elements (columns_batch changes nothing):
 *    output[i] = vec_a[i] * vec_b[i]^-1. The inverse of zero is zero, so a / 0 = 0 and inv(0) = 0, and a zero disturbs no other
 *    element. In place is allowed (output == vec_a, for vector_div also output == vec_b); partial overlap is undefined.
 *    The elements of a tile of icicle_hip_vector_inv_tile(words) neighbours share one a^(p-2) chain (Montgomery's trick).
 *  - vector_sum / vector_product write batch_size contiguous elements: entry k reduces its elements j < size, found at
 *    k * size + j, or at j * batch_size + k with columns_batch. The result is the same bytes on every run.
 *  - config: is_a_on_device, is_b_on_device, is_result_on_device, stream and is_async as for vector_mul. NULL config gives
 *    ICICLE_INVALID_POINTER, then size == 0 gives ICICLE_SUCCESS with nothing written, then a NULL vector ICICLE_INVALID_POINTER. */
#define ICICLE_HIP_DECLARE_VEC_INV(F)                                                                                  \
  icicle_error_t F##_vector_inv(const void* vec_a, uint64_t size, const icicle_vec_ops_config_t* config, void* output); \
  icicle_error_t F##_vector_div(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* output); \
  icicle_error_t F##_vector_sum(const void* vec_a, uint64_t size, const icicle_vec_ops_config_t* config, void* output); \
  icicle_error_t F##_vector_product(const void* vec_a, uint64_t size, const icicle_vec_ops_config_t* config, void* output);
ICICLE_HIP_DECLARE_VEC_INV(babybear)
ICICLE_HIP_DECLARE_VEC_INV(koalabear)
ICICLE_HIP_DECLARE_VEC_INV(bn254)
ICICLE_HIP_DECLARE_VEC_INV(bls12_381)
/* elements that share one inversion, for elements of 1, 2 or 8 words; 0 for any other width. Needs no device. */
int icicle_hip_vector_inv_tile(int words_per_element);

/* The same operations over the extension field, for the three fields that have an extension type: babybear, koalabear, goldilocks
 * (src/vec_ops.cpp:24-64 extension_vector_product / _sum, :87-97 _vector_add, :152-162 _vector_sub, :185-210 _vector_mul and
 * _vector_mixed_mul, :233-243 _vector_div, :265-274 _vector_inv, :297-315 _scalar_add_vec, :338-356 _scalar_sub_vec, :378-396
 * _scalar_mul_vec, :455-464 _bit_reverse; cmake/features.cmake EXT_FIELD).
 *  - An element is 16 bytes. babybear, koalabear: four canonical 4-byte coefficients, constant term first, of F[x] / (x^4 - W),
 *    W = 11 and 3. goldilocks: two canonical 8-byte coefficients c0 + c1 u, u^2 = 7.
 *  - Semantics, config and argument checks are those of the base-field functions above, over extension elements: `size` is per
 *    batch entry, scalar_*_vec take one extension scalar per batch entry (scalar_sub_vec is scalar minus vector), columns_batch
 *    matters to them and to sum / product only, in place is allowed, inv(0) = 0 and a / 0 = 0, sum and product give the same bytes
 *    on every run. vector_mixed_mul multiplies an extension vector by a BASE-field vector (4 or 8 bytes per element of vec_b).
 *    extension_bit_reverse checks its arguments as bit_reverse does.
 *  - vector_inv / vector_div take the norm of each element down to the base field; the norms of a tile of
 *    icicle_hip_extension_vector_inv_tile(base words) neighbours share one base-field a^(p-2) chain. */
#define ICICLE_HIP_DECLARE_VEC_EXT(F)                                                                                  \
  icicle_error_t F##_extension_vector_add(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_vector_sub(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_vector_mul(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_vector_div(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_vector_mixed_mul(const void* vec_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_vector_inv(const void* vec_a, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_vector_sum(const void* vec_a, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_vector_product(const void* vec_a, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_scalar_add_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_scalar_sub_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_scalar_mul_vec(const void* scalar_a, const void* vec_b, uint64_t size, const icicle_vec_ops_config_t* config, void* result); \
  icicle_error_t F##_extension_bit_reverse(const void* input, uint64_t size, const icicle_vec_ops_config_t* config, void* output);
ICICLE_HIP_DECLARE_VEC_EXT(babybear)
ICICLE_HIP_DECLARE_VEC_EXT(koalabear)
ICICLE_HIP_DECLARE_VEC_EXT(goldilocks)
/* elements whose norms share one inversion, by the words of a BASE-field element (1 or 2); 0 for anything else. Needs no device. */
int icicle_hip_extension_vector_inv_tile(int base_words_per_element);

/* slice, highest_non_zero_idx, poly_eval and poly_division: what the reference's polynomial API is built from, for the eight fields
 * above (src/vec_ops.cpp:472 slice, :549 highest_non_zero_idx, :621 poly_eval, :648 poly_division; CPU backend
 * backend/cpu/src/field/cpu_vec_ops.cpp:566-624, 682-780). Elements are canonical words in and out. Every size is per batch entry:
 * entry k holds its element j at k * size + j, or at j * batch_size + k with columns_batch. stream, is_async and the three
 * is_*_on_device flags are honoured as vector_div honours them. Arguments are checked before the device is touched, in vector_inv's
 * order: NULL config gives ICICLE_INVALID_POINTER, then the empty call named below ICICLE_SUCCESS, then a NULL vector
 * ICICLE_INVALID_POINTER, then everything else ICICLE_INVALID_ARGUMENT.
 *  - slice: output[k][i] = input[k][offset + i * stride], i < size_out. size_out == 0 is the empty call.
 *    offset + (size_out - 1) * stride >= size_in is an error (where the reference asserts), also with stride == 0. Input and output
 *    must not overlap: an overlap of two buffers on the same side (host or device) is an error, nothing is written.
 *  - highest_non_zero_idx: out_idx[k] = the largest j whose element has a non-zero word, -1 for a zero vector; batch_size int64_t
 *    values, on the device with is_result_on_device. size == 0 is an error. A maximum of integers: the same on every run.
 *  - poly_eval: evals[k][e] = P_k(domain[e]). The domain is shared by the entries and contiguous; coeffs (is_a_on_device) and evals
 *    (is_result_on_device) follow columns_batch; is_b_on_device is the domain's. coeffs_size == 0 or domain_size == 0 is an error.
 *    evals must overlap neither input. Two routes with the same bytes out: one lane per (entry, point), or -- few points, many
 *    coefficients -- one wave per chunk of coefficients and further launches over the chunk values. config.ext int
 *    "hip_poly_eval_chunk": absent or 0 the plan decides (csrc/poly_plan.h), positive the chunk route with that chunk length (1 is
 *    taken as 2), -1 the point route, any other negative value is an error.
 *  - poly_division: numerator = q * denominator + r per entry. q_out gets q_size elements per entry and r_out r_size, both written in
 *    full, zero above the quotient's and the remainder's degree. With deg = highest_non_zero_idx: a zero denominator in any entry,
 *    r_size < deg_n + 1, and q_size < deg_n - deg_b + 1 where that is positive are errors, and nothing is written. deg_n < deg_b gives
 *    q = 0 and r = numerator; a zero numerator gives zeros. The outputs may overlap neither the inputs nor each other.
 *    is_a_on_device is the numerator's, is_b_on_device the denominator's, is_result_on_device covers q_out and r_out. The call
 *    synchronises the stream once, to read the degrees. The quotient is produced from the top in tiles of
 *    icicle_hip_poly_division_tile(words) coefficients, two launches per tile. */
#define ICICLE_HIP_DECLARE_VEC_POLY(F)                                                                                 \
  icicle_error_t F##_slice(const void* input, uint64_t offset, uint64_t stride, uint64_t size_in, uint64_t size_out, const icicle_vec_ops_config_t* config, void* output); \
  icicle_error_t F##_highest_non_zero_idx(const void* input, uint64_t size, const icicle_vec_ops_config_t* config, int64_t* out_idx); \
  icicle_error_t F##_poly_eval(const void* coeffs, uint64_t coeffs_size, const void* domain, uint64_t domain_size, const icicle_vec_ops_config_t* config, void* evals); \
  icicle_error_t F##_poly_division(const void* numerator, uint64_t numerator_size, const void* denominator, int64_t denominator_size, const icicle_vec_ops_config_t* config, \
                                   void* q_out, uint64_t q_size, void* r_out, uint64_t r_size);
ICICLE_HIP_DECLARE_VEC_POLY(babybear)
ICICLE_HIP_DECLARE_VEC_POLY(koalabear)
ICICLE_HIP_DECLARE_VEC_POLY(goldilocks)
ICICLE_HIP_DECLARE_VEC_POLY(bn254)
ICICLE_HIP_DECLARE_VEC_POLY(bls12_381)
ICICLE_HIP_DECLARE_VEC_POLY(bls12_377)
ICICLE_HIP_DECLARE_VEC_POLY(stark252)
ICICLE_HIP_DECLARE_VEC_POLY(grumpkin)
/* quotient coefficients per tile of poly_division, for elements of 1, 2 or 8 words; 0 for any other width. Needs no device. */
int icicle_hip_poly_division_tile(int words_per_element);

/* Matrix transpose of batch_size row-major nof_rows x nof_cols matrices (icicle/src/matrix_ops.cpp:75-102,
 * include/icicle/vec_ops.h:319; CPU: backend/cpu/src/field/cpu_matrix_ops.cpp:333-362): in place allowed, columns_batch
 * rejected. The Rust NTT suite calls it on the main device around every columns_batch transform
 * (wrappers/rust/icicle-core/src/ntt/tests.rs:311-335). */
#define ICICLE_HIP_DECLARE_TRANSPOSE(F, S)                                                                             \
  icicle_error_t F##_##S(const void* mat_in, uint32_t nof_rows, uint32_t nof_cols, const icicle_vec_ops_config_t* config, void* mat_out); \
  icicle_error_t icicle_hip_##F##_##S(const void* mat_in, uint32_t nof_rows, uint32_t nof_cols, const icicle_vec_ops_config_t* config, void* mat_out);
ICICLE_HIP_DECLARE_TRANSPOSE(babybear, matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(koalabear, matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(babybear, extension_matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(koalabear, extension_matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(goldilocks, matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(goldilocks, extension_matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(bn254, matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(bls12_381, matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(bls12_377, matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(grumpkin, matrix_transpose)
ICICLE_HIP_DECLARE_TRANSPOSE(stark252, matrix_transpose)

/* ======================================================================================
 * Hash + Merkle tree: src/hash/hash_c_api.cpp:22-139 (icicle_hasher_*, icicle_create_keccak_256 / _512, icicle_create_sha3_256 / _512,
 * icicle_create_blake2s, icicle_create_blake3),
 * src/hash/merkle_c_api.cpp:12-166 (icicle_merkle_proof_*, icicle_merkle_tree_*), include/icicle/hash/hash_config.h:15-24
 * (HashConfig, 32 bytes), include/icicle/merkle/merkle_tree_config.h:11-37 (PaddingPolicy, MerkleTreeConfig, 24 bytes).
 * Keccak-f[1600] sponges: rate 136 bytes for the 256-bit digests, 72 bytes for the 512-bit ones; Keccak pads 0x01 .. 0x80,
 * SHA3 0x06 .. 0x80. Creating and deleting handles needs no GPU; hashing, build, get_proof and verify run on the device and
 * fail without one. Blake2s-256 and Blake3 hash through the same entry points; the proof-of-work solver and verifier over all six
 * hashers follow the Merkle functions below, and FRI over every field with an NTT, which composes all of them, follows the proof of work;
 * sumcheck, whose transcript hashes through the same entry points, follows FRI; execute_program, which runs the same programs over
 * vectors, follows sumcheck.
 * Poseidon2 over BabyBear and KoalaBear hashes and builds trees through the same entry points (its factories follow the Blake ones).
 * Poseidon over the scalar fields of BN254, BLS12-381, BLS12-377 and Grumpkin does the same (its factories follow Poseidon2's).
 * Poseidon2 over the same four fields and stark252, of width 2, 3, 4, 8, does the same (its factories follow Poseidon's).
 * Poseidon over the other fields and in sponge mode, Poseidon2 over Goldilocks and M31, proof serialisation (Merkle, FRI and sumcheck) and the extension_ / rns_
 * variants of execute_program are not built.
 * ====================================================================================== */
typedef struct {
  icicleStreamHandle stream;      /* 0  */
  uint64_t batch;                 /* 8   messages per call */
  bool are_inputs_on_device;      /* 16 */
  bool are_outputs_on_device;     /* 17 */
  bool is_async;                  /* 18 */
  icicle_config_extension_t* ext; /* 24  foreign keys ("n_threads" of the CPU backend) are ignored */
} icicle_hash_config_t;

enum { ICICLE_PADDING_NONE = 0, ICICLE_PADDING_ZERO = 1, ICICLE_PADDING_LAST_VALUE = 2 }; /* merkle_tree_config.h:11-15 */
typedef struct {
  icicleStreamHandle stream;      /* 0  */
  bool is_leaves_on_device;       /* 8  */
  bool is_tree_on_device;         /* 9   stored layers stay in device memory (otherwise pinned host memory) */
  bool is_async;                  /* 10 */
  int padding_policy;             /* 12  ICICLE_PADDING_* */
  icicle_config_extension_t* ext; /* 16  "hip_merkle_top_max_hashes" (int): layers with at most this many hashes, and all above them,
                                         run in ONE launch (default 1024; 0 = one launch per layer) */
} icicle_merkle_tree_config_t;

typedef struct icicle_hasher* icicle_hasher_handle_t;
typedef struct icicle_merkle_tree* icicle_merkle_tree_handle_t;
typedef struct icicle_merkle_proof* icicle_merkle_proof_handle_t;

/* input_chunk_size: the default message size of the hasher (0 = none) -- the size of one input of a Merkle tree layer */
icicle_hasher_handle_t icicle_create_keccak_256(uint64_t input_chunk_size); /* hash_c_api.cpp:71 */
icicle_hasher_handle_t icicle_create_keccak_512(uint64_t input_chunk_size); /* :84 */
icicle_hasher_handle_t icicle_create_sha3_256(uint64_t input_chunk_size);   /* :97 */
icicle_hasher_handle_t icicle_create_sha3_512(uint64_t input_chunk_size);   /* :110 */
/* Blake2s-256 (RFC 7693, no key) and Blake3 (default hash mode, 32-byte output; any message length) */
icicle_hasher_handle_t icicle_create_blake2s(uint64_t input_chunk_size);    /* :123 */
icicle_hasher_handle_t icicle_create_blake3(uint64_t input_chunk_size);     /* :136 */
/* Poseidon2 (src/hash/poseidon2_c_api.cpp:13, semantics of backend/cpu/src/hash/cpu_poseidon2.cpp) of width t in {2, 3, 4, 8, 12, 16,
 * 20, 24} over a 31-bit field; NULL for any other width. Elements are 4-byte canonical residues, the digest is one element (4 bytes:
 * state[1]). domain_tag: NULL, or one element that becomes state[0]. input_size: the default message size in elements (a Merkle
 * layer's input), 0 = one permutation's worth: t, or t - 1 beside a tag. A message of exactly that many elements is one
 * permutation. Any other size is a sponge over a zero state: state[0] is the tag or else the first element, the rest is added into
 * state[1 .. t-1], t - 1 elements per permutation; only an incomplete last block is padded, with 1, 0, 0, ..; fewer than t elements
 * are one permutation. icicle_hasher_hash wants input_len % 4 == 0 and device operands 4-aligned (INVALID_ARGUMENT otherwise);
 * proof_of_work and proof_of_work_verify refuse these hashers (INVALID_ARGUMENT). alpha, the round numbers, the round constants
 * and the internal matrix are derived from the specification when the hasher is created (icicle_amd/csrc/poseidon2_params.h), on
 * the host; they are uploaded when the hasher first hashes on a device and freed with the hasher and the trees that copied it. */
icicle_hasher_handle_t babybear_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
icicle_hasher_handle_t koalabear_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
/* Poseidon (src/hash/poseidon_c_api.cpp, semantics of backend/cpu/src/hash/cpu_poseidon.cpp) of width t in {3, 5, 9, 12} over the
 * scalar field of BN254, BLS12-381, BLS12-377 or Grumpkin: S-box x^5, 8 full rounds, 56 / 56 / 57 / 57 partial rounds, the Cauchy
 * matrix 1 / (i + j + t), round constants from the Grain LFSR. Elements are 8 little-endian 32-bit words, canonical; the digest is
 * one element (32 bytes: state[1]). domain_tag: NULL, or one element (8 words) that becomes state[0]; the arity is t, or t - 1
 * beside a tag. input_size: 0 or the arity. NULL for any other width, for bls12_381 at t = 3 (the reference has no defined result
 * there), for a tag >= p and for any other input_size. icicle_hasher_hash takes messages of exactly 32 * arity bytes and answers
 * INVALID_ARGUMENT to any other length: the reference refuses longer messages and reads past the end of shorter ones, so shorter
 * ones are refused here. Device operands 4-aligned. proof_of_work and proof_of_work_verify refuse these hashers
 * (INVALID_ARGUMENT). The tables of the optimized schedule are derived when the hasher is created
 * (icicle_amd/csrc/poseidon_params.h), on the host; they are uploaded when a hasher of that (field, t) first hashes on a device. */
icicle_hasher_handle_t bn254_create_poseidon_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
icicle_hasher_handle_t bls12_381_create_poseidon_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
icicle_hasher_handle_t bls12_377_create_poseidon_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
icicle_hasher_handle_t grumpkin_create_poseidon_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
/* Poseidon2 (the same entry of the reference, built per field) of width t in {2, 3, 4, 8} over the scalar field of BN254, BLS12-381,
 * BLS12-377 or Grumpkin or over stark252; NULL for any other width (the reference's tables for these fields end at 8) and for a
 * tag >= p. S-box x^5 (x^11 for BLS12-377, x^3 for stark252), 8 full rounds, 56 / 56 / 56 / 57 partial rounds (37 for BLS12-377,
 * 83 / 83 / 84 / 84 for stark252). Elements are 8 little-endian 32-bit words, canonical; the digest is one element (32 bytes:
 * state[1]). domain_tag: NULL, or one element (8 words) that becomes state[0]. input_size and the exact-arity / sponge rule are
 * those of the 31-bit factories above, counted in elements of 32 bytes. icicle_hasher_hash wants input_len % 32 == 0
 * (INVALID_ARGUMENT otherwise, before the device is touched) and device operands 4-aligned; proof_of_work and
 * proof_of_work_verify refuse these hashers (INVALID_ARGUMENT). alpha, the round numbers, the round constants and the internal
 * matrix are derived from the specification when the first hasher of a (field, t) is created
 * (icicle_amd/csrc/poseidon2_wide_params.h), on the host, and kept for the process; they are uploaded when a hasher of that
 * pair first hashes on a device. */
icicle_hasher_handle_t bn254_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
icicle_hasher_handle_t bls12_381_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
icicle_hasher_handle_t bls12_377_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
icicle_hasher_handle_t grumpkin_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
icicle_hasher_handle_t stark252_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
/* Poseidon2 (the same entry of the reference, built for Goldilocks) of width t in {2, 3, 4, 8, 12, 16, 20, 24} over p = 2^64 - 2^32 + 1;
 * NULL for any other width and for a tag >= p. S-box x^7, 8 full rounds, 27 / 23 / 21 partial rounds at t = 2, 3, 4 and 22 from
 * t = 8 on. Elements are 8-byte canonical residues (two little-endian 32-bit words; an input word in [p, 2^64) is brought below
 * p), the digest is one element (8 bytes: state[1]). domain_tag: NULL, or one element (2 words) that becomes state[0]. input_size
 * and the exact-arity / sponge rule are those of the 31-bit factories above, counted in elements of 8 bytes. icicle_hasher_hash
 * wants input_len % 8 == 0 (INVALID_ARGUMENT otherwise, before the device is touched) and device operands 8-aligned;
 * proof_of_work and proof_of_work_verify refuse these hashers (INVALID_ARGUMENT). alpha, the round numbers, the round constants
 * and the internal matrix are derived from the specification when the first hasher of a width is created
 * (icicle_amd/csrc/poseidon2_gold_params.h), on the host, and kept for the process; they are uploaded when the hasher first
 * hashes on a device and freed with the hasher and the trees that copied it. */
icicle_hasher_handle_t goldilocks_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size);
/* config->batch messages of input_len bytes each, back to back (input_len = 0: the hasher's default chunk size; both 0:
 * INVALID_ARGUMENT); digests of 32 / 64 bytes back to back. Any length, any pointer alignment (Poseidon2: see its factories). */
icicle_error_t icicle_hasher_hash(icicle_hasher_handle_t h, const uint8_t* input, uint64_t input_len, const icicle_hash_config_t* config, uint8_t* output); /* :22 */
uint64_t icicle_hasher_output_size(icicle_hasher_handle_t h); /* :40 */
icicle_error_t icicle_hasher_delete(icicle_hasher_handle_t h); /* :52 */

/* Layer i hashes n_i inputs of c_i bytes (its hasher's chunk size) into digests of o_i bytes: c_{i+1} % o_i == 0 is required
 * (NULL otherwise), n_{L-1} = 1, n_{i-1} = n_i * c_i / o_{i-1}, the tree takes n_0 * c_0 bytes of leaves. The tree copies the
 * hashers. Layers >= output_store_min_layer are kept (device or pinned host memory per is_tree_on_device), lower ones are
 * freed after the build and re-hashed, one sub-tree per opening (get_proofs: per distinct sub-tree), from the caller's leaves. */
icicle_merkle_tree_handle_t icicle_merkle_tree_create(const icicle_hasher_handle_t* layer_hashes, size_t layer_hashes_len, uint64_t leaf_element_size,
                                                      uint64_t output_store_min_layer); /* merkle_c_api.cpp:75 */
icicle_error_t icicle_merkle_tree_delete(icicle_merkle_tree_handle_t tree);             /* :103 */
/* The tree over the leaves padded to n_0 * c_0 bytes: ZeroPadding appends zeros, LastValue repeats the last leaf_element_size
 * bytes (size and c_0 must be multiples of leaf_element_size). INVALID_ARGUMENT: size 0, size beyond the capacity, short leaves
 * with policy None, a second build. */
icicle_error_t icicle_merkle_tree_build(icicle_merkle_tree_handle_t tree, const uint8_t* leaves, uint64_t size, const icicle_merkle_tree_config_t* config); /* :111 */
/* Host pointer owned by the tree (NULL before build). After a build with is_async the bytes are valid once the caller has
 * synchronised the build's stream. */
const uint8_t* icicle_merkle_tree_get_root(icicle_merkle_tree_handle_t tree, size_t* out_size); /* :124 */
/* Proof for element leaf_idx (cpu_merkle_tree.cpp:143-211,546-573): leaf = the whole layer-0 chunk around the element, padded per
 * policy; path = for layers 0 .. L-2 the c_{i+1} bytes of layer-i digests that form the on-path input of layer i+1 (pruned: without
 * the on-path digest itself). leaf_idx * leaf_element_size beyond the capacity, or a tree not built: INVALID_ARGUMENT. Synchronises
 * config->stream once. This is icicle_hip_merkle_tree_get_proofs (below) with count == 1: the same code, refusals and bytes. */
icicle_error_t icicle_merkle_tree_get_proof(icicle_merkle_tree_handle_t tree, const uint8_t* leaves, uint64_t leaves_size, uint64_t leaf_idx, bool is_pruned,
                                            const icicle_merkle_tree_config_t* config, icicle_merkle_proof_handle_t merkle_proof); /* :138 */
/* include/icicle/merkle/merkle_tree.h:148-203, one hash per layer on the device: icicle_hip_merkle_tree_verify_batch (below) with
 * count == 1, the same code, refusals and verdict */
icicle_error_t icicle_merkle_tree_verify(icicle_merkle_tree_handle_t tree, icicle_merkle_proof_handle_t merkle_proof, bool* valid); /* :157 */
icicle_merkle_proof_handle_t icicle_merkle_proof_create(void); /* :12 */
icicle_merkle_proof_handle_t icicle_merkle_proof_create_with_data(bool pruned_path, int64_t leaf_idx, const uint8_t* leaf, size_t leaf_size, const uint8_t* root,
                                                                  size_t root_size, const uint8_t* path, size_t path_size); /* :15 */
icicle_error_t icicle_merkle_proof_delete(icicle_merkle_proof_handle_t proof);  /* :32 */
bool icicle_merkle_proof_is_pruned(icicle_merkle_proof_handle_t proof);         /* :40 */
const uint8_t* icicle_merkle_proof_get_path(icicle_merkle_proof_handle_t proof, size_t* out_size); /* :47 */
const uint8_t* icicle_merkle_proof_get_leaf(icicle_merkle_proof_handle_t proof, size_t* out_size, uint64_t* out_leaf_idx); /* :56 */
const uint8_t* icicle_merkle_proof_get_root(icicle_merkle_proof_handle_t proof, size_t* out_size); /* :66 */

/* ---- this backend's own: many openings, many verifications per call (the reference has no such call). The single calls above are
 * these two with count == 1; there is one implementation of each. ----
 * get_proofs: proofs[i] comes out byte for byte as icicle_merkle_tree_get_proof(tree, leaves, leaves_size, leaf_indices[i], is_pruned,
 * config, proofs[i]) leaves it, for every configuration that call accepts. leaf_indices is a host array, in any order, repeats
 * allowed; proofs are `count` handles of icicle_merkle_proof_create. With the stored layers in device memory ONE kernel gathers the
 * on-path groups of all proofs (and, for device leaves, the leaf chunks and the LastValue element) into count staging records,
 * which come back in one copy into pinned memory behind the one synchronisation of config->stream (is_async or not); pieces that
 * live on the host (a tree in pinned memory, host leaves) are copied on the host. Launches, copies and synchronisations do not
 * grow with count; with output_store_min_layer > 0 the layers below it are re-hashed once per DISTINCT sub-tree among the indices.
 * NULL tree, config, leaves, leaf_indices, proofs or proofs[i]: INVALID_POINTER. A tree not built, leaves the tree's build would refuse,
 * any index at or beyond the capacity, count * (bytes of one proof's pieces) beyond 2^40: INVALID_ARGUMENT. Both before the device is touched,
 * and with every proof object untouched. count == 0: SUCCESS, nothing done. */
icicle_error_t icicle_hip_merkle_tree_get_proofs(icicle_merkle_tree_handle_t tree, const uint8_t* leaves, uint64_t leaves_size, const uint64_t* leaf_indices, uint64_t count,
                                                 bool is_pruned, const icicle_merkle_tree_config_t* config, icicle_merkle_proof_handle_t* proofs);
/* valid[i] = what icicle_merkle_tree_verify(tree, proofs[i], &v) would set. One upload of all proofs' layer inputs, one hash launch
 * per layer over all proofs (layer 0: one per distinct leaf size), pruned proofs' digests scattered into the next layer's inputs by
 * one launch per layer, one copy back, one synchronisation (the null stream); the comparisons run on the host.
 * All proofs share one pruned flag: a mix is INVALID_ARGUMENT. Where some proof is refused (an empty leaf, a path of the wrong
 * size, leaf_idx * leaf_element_size beyond 64 bits: INVALID_ARGUMENT) the call returns the first such error in index order and
 * every valid[i] is false. A root of the wrong size makes that one proof invalid. NULL tree, proofs, valid or proofs[i]:
 * INVALID_POINTER. count == 0: SUCCESS. The tree need not be built. */
icicle_error_t icicle_hip_merkle_tree_verify_batch(icicle_merkle_tree_handle_t tree, const icicle_merkle_proof_handle_t* proofs, uint64_t count, bool* valid);

/* ---- proof of work: include/icicle/hash/pow.h:16-87 (PowConfig, 32 bytes; proof_of_work, proof_of_work_verify), semantics
 * backend/cpu/src/hash/cpu_pow.cpp. `const Hash&` and the `bool&` / `uint64_t&` results cross the ABI as pointers
 * (wrappers/rust/icicle-hash/src/pow.rs:28-53). The message of nonce n is challenge[0, challenge_size) | n as 8 little-endian
 * bytes | padding_size zero bytes; its candidate is the first 8 digest bytes as a little-endian word; n solves when the candidate
 * is below 2^(64 - solution_bits). ---- */
typedef struct {
  icicleStreamHandle stream;      /* 0  */
  bool is_challenge_on_device;    /* 8  */
  uint32_t padding_size;          /* 12  default 24: a 32-byte challenge makes a 64-byte message */
  bool is_async;                  /* 16  accepted and ignored: the results are host scalars, so both calls return with `stream` drained */
  icicle_config_extension_t* ext; /* 24  all ints, all optional, foreign keys ignored:
                                         "hip_pow_span_log2"  nonces per kernel launch, 0 .. 32 (default for a message of one hash block: 22 for the
                                                              Keccak / SHA3 hashers, 24 for Blake2s / Blake3; one less per doubling of
                                                              its blocks, at least 16)
                                         "hip_pow_start_lo", "hip_pow_start_hi"  first nonce tried, hi << 32 | (uint32_t)lo (default 0)
                                         "hip_pow_count_log2" nonces tried from the first one, 0 .. 64 (default 64: all of them) */
} icicle_pow_config_t;

/* The SMALLEST solving nonce among those tried, counting up from the first, and its candidate: *found = true, *nonce, *mined_hash.
 * The nonces tried end at 2^64 - 1024, where the reference's loop of 1024-nonce rounds ends. When none solves: *found = false,
 * *nonce and *mined_hash untouched. hasher: any of the six of icicle_create_*; Blake3 only while challenge_size + 8 + padding_size
 * <= 1024 (one chunk), INVALID_ARGUMENT beyond. solution_bits outside 1 .. 60, or a key above out of range: INVALID_ARGUMENT. NULL
 * hasher, config or result pointer, NULL challenge with challenge_size > 0: INVALID_POINTER. Argument errors are returned before the
 * device is touched. The challenge may lie at any address, on the host or (is_challenge_on_device) on the device. */
icicle_error_t proof_of_work(icicle_hasher_handle_t hasher, const uint8_t* challenge, uint32_t challenge_size, uint8_t solution_bits, const icicle_pow_config_t* config,
                             bool* found, uint64_t* nonce, uint64_t* mined_hash); /* pow.h:52 */
/* One hash: *mined_hash = the candidate of `nonce`, *is_correct = it is below the threshold. Same argument errors. */
icicle_error_t proof_of_work_verify(icicle_hasher_handle_t hasher, const uint8_t* challenge, uint32_t challenge_size, uint8_t solution_bits,
                                    const icicle_pow_config_t* config, uint64_t nonce, bool* is_correct, uint64_t* mined_hash); /* pow.h:79 */

/* ---- FRI over BabyBear and KoalaBear, scalar (F = S = one word) and quartic extension (F = 4 words, S = the base field):
 * src/fri/fri_c_api.cpp:76-312 (scalar) and :314-563 (P_extension_), include/icicle/fri/fri_config.h:16-25 (FriConfig, 56 bytes),
 * fri_c_api.cpp:13-32 (FFIFriTranscriptConfig, 96 bytes); protocol src/fri/fri.cpp, include/icicle/fri/fri_transcript.h,
 * backend/cpu/include/cpu_fri_backend.h. Every layer of the commit phase lives in device memory: round r builds its tree
 * (icicle_merkle_tree_build, leaves and tree on the device) over n >> r elements -- leaves hasher with chunk = one element, then
 * log2(n) - r layers of the compress hasher --, hashes the transcript with icicle_hasher_hash, and folds with the challenge:
 *   out[i] = (e[i] + e[i+h])/2 + alpha * ((e[i] - e[i+h])/2 * w_n^(-i)),  h = n/2,  w_n^(-i) from the initialised NTT domain.
 * The last fold's output is the final polynomial; proof_of_work (default config) grinds pow_bits; the query phase opens
 * q % (n>>r) and its symmetric position (q + (n>>r)/2) % (n>>r) in every round, not pruned, with ONE icicle_hip_merkle_tree_get_proofs per round.
 * Queries come from a hand-written MT19937 seeded with the low 32 bits of the transcript digest (icicle_amd/csrc/fri_plan.h), so a
 * proof does not depend on the C++ library. A proof stores 2 * nof_queries slots (query, symmetric); get_nof_queries returns that
 * doubled number. The MerkleProof handles of get_round_proofs_for_query are borrowed from the proof and work with
 * icicle_merkle_proof_get_*. The three serialisation functions are not built.
 * INVALID_ARGUMENT, before the device is touched: folding_factor != 2, input_size zero or no power of two, nof_queries == 0 or
 * > input_size / 2, compress arity (chunk / output size) != 2, and -- left undefined by the reference, whose final polynomial then
 * stays zero -- stopping_degree + 1 no power of two or zero rounds (stopping_degree + 1 >= input_size). Two more of this backend: a
 * leaves hasher whose chunk is not one element (4 or 16 bytes; the reference's tree build fails there), and pow_bits > 60
 * (proof_of_work's range). A domain that is missing or smaller than input_size: INVALID_ARGUMENT. NULL config, transcript, hasher,
 * seed, input or proof: INVALID_POINTER. The caller keeps the domain alive (no ntt_release_domain) until prove has returned.
 * `stream` is honoured, is_async accepted; prove returns with the stream drained (the proof is host data), as proof_of_work does.
 * verify: final-polynomial length, alphas from the proof's roots, proof of work, then per round all Merkle proofs
 * (one icicle_hip_merkle_tree_verify_batch), then per query and round leaf indices, collinearity with w_n^(-1) from the field's own root of unity. The argument errors above
 * that concern the configuration and the hashers are errors in verify too; everything about the proof itself -- its final polynomial's
 * length, a number of slots other than 2 * nof_queries, rounds that differ between slots, a size 2^rounds * final size that does not
 * fit nof_queries, words at or above p -- makes a wrong proof: *valid = false with SUCCESS. Stricter than the reference in one point:
 * every slot of a round must carry the same root as slot 0, from which the round's challenge is derived (the reference compares each
 * Merkle proof only with the root that proof itself carries). ---- */
typedef struct {
  icicleStreamHandle stream;      /* 0  */
  size_t folding_factor;          /* 8   only 2 */
  size_t stopping_degree;         /* 16  the final polynomial has stopping_degree + 1 coefficients */
  size_t pow_bits;                /* 24  0 = no proof of work (default 16) */
  size_t nof_queries;             /* 32  (default 100) */
  bool are_inputs_on_device;      /* 40 */
  bool is_async;                  /* 41 */
  icicle_config_extension_t* ext; /* 48 */
} icicle_fri_config_t;
typedef struct {
  icicle_hasher_handle_t hasher;         /* 0  */
  const uint8_t* domain_separator_label; /* 8  */
  size_t domain_separator_label_len;     /* 16 */
  const uint8_t* round_challenge_label;  /* 24 */
  size_t round_challenge_label_len;      /* 32 */
  const uint8_t* commit_phase_label;     /* 40 */
  size_t commit_phase_label_len;         /* 48 */
  const uint8_t* nonce_label;            /* 56 */
  size_t nonce_label_len;                /* 64 */
  const uint8_t* public_state;           /* 72 */
  size_t public_state_len;               /* 80 */
  const uint32_t* seed_rng;              /* 88  one element of F, canonical */
} icicle_fri_transcript_config_t;
typedef struct icicle_fri_proof* icicle_fri_proof_handle_t;
#define ICICLE_HIP_DECLARE_FRI(P)                                                                                      \
  icicle_fri_proof_handle_t P##_icicle_initialize_fri_proof(void);                                                     \
  icicle_fri_proof_handle_t P##_icicle_create_with_arguments_fri_proof(icicle_merkle_proof_handle_t** query_proofs, size_t nof_queries, size_t nof_rounds, \
                                                                       const uint32_t* final_poly, size_t final_poly_size, uint64_t pow_nonce); \
  icicle_error_t P##_icicle_delete_fri_proof(icicle_fri_proof_handle_t proof);                                         \
  icicle_error_t P##_fri_proof_get_nof_queries(icicle_fri_proof_handle_t proof, size_t* nof_queries);                  \
  icicle_error_t P##_fri_proof_get_nof_rounds(icicle_fri_proof_handle_t proof, size_t* nof_rounds);                    \
  icicle_error_t P##_fri_proof_get_round_proofs_for_query(icicle_fri_proof_handle_t proof, size_t query_idx, icicle_merkle_proof_handle_t* proofs); \
  icicle_error_t P##_fri_proof_get_final_poly_size(icicle_fri_proof_handle_t proof, size_t* result);                   \
  icicle_error_t P##_fri_proof_get_final_poly(icicle_fri_proof_handle_t proof, uint32_t** final_poly);                 \
  icicle_error_t P##_fri_proof_get_pow_nonce(icicle_fri_proof_handle_t proof, uint64_t* result);                       \
  icicle_error_t P##_fri_merkle_tree_prove(const icicle_fri_config_t* fri_config, const icicle_fri_transcript_config_t* transcript_config, const uint32_t* input_data, \
                                           size_t input_size, icicle_hasher_handle_t merkle_tree_leaves_hash, icicle_hasher_handle_t merkle_tree_compress_hash, \
                                           uint64_t output_store_min_layer, icicle_fri_proof_handle_t fri_proof);      \
  icicle_error_t P##_fri_merkle_tree_verify(const icicle_fri_config_t* fri_config, const icicle_fri_transcript_config_t* transcript_config, icicle_fri_proof_handle_t fri_proof, \
                                            icicle_hasher_handle_t merkle_tree_leaves_hash, icicle_hasher_handle_t merkle_tree_compress_hash, bool* valid); \
  /* backend-specific: one fold of n = 2^k elements into n / 2 (in, out and alpha on the host or all three on the device);        \
   * INVALID_ARGUMENT: n no power of two, n < 2, the domain missing or smaller than n */                                         \
  icicle_error_t P##_hip_fri_fold(const uint32_t* in, uint64_t n, const uint32_t* alpha, uint32_t* out, bool on_device, icicleStreamHandle stream);
ICICLE_HIP_DECLARE_FRI(babybear)
ICICLE_HIP_DECLARE_FRI(babybear_extension)
ICICLE_HIP_DECLARE_FRI(koalabear)
ICICLE_HIP_DECLARE_FRI(koalabear_extension)
/* The same over the wider fields that have an NTT, with the same functions, structs and rules: Goldilocks (an element is 8 bytes)
 * and its quadratic extension (16 bytes: a0 + a1 u with u^2 = 7, constant term first), stark252 and the scalar fields of BN254,
 * BLS12-381 and BLS12-377 (32 bytes). Elements are canonical little-endian words; the leaves hasher's chunk is one element (8, 16 or
 * 32 bytes), seed_rng is one element. F(digest) is the reference's from(bytes, size): a scalar is the whole digest as one
 * little-endian integer mod p, an extension element takes coefficient k from bytes 8k .. 8k+7 mod p. The twiddles come from the
 * domain of <field>_ntt_init_domain on the current device (goldilocks_extension uses goldilocks'). */
ICICLE_HIP_DECLARE_FRI(goldilocks)
ICICLE_HIP_DECLARE_FRI(goldilocks_extension)
ICICLE_HIP_DECLARE_FRI(stark252)
ICICLE_HIP_DECLARE_FRI(bn254)
ICICLE_HIP_DECLARE_FRI(bls12_381)
ICICLE_HIP_DECLARE_FRI(bls12_377)

/* ---- Sumcheck, programs and symbols: src/sumcheck/sumcheck_c_api.cpp, src/program/program_c_api.cpp, src/symbol/symbol_api.cpp,
 * include/icicle/sumcheck/sumcheck_config.h (SumcheckConfig, 40 bytes), TranscriptConfigFFI (72 bytes). Over babybear, koalabear
 * (one word per element) and the bn254, bls12_381 scalar fields (eight words), canonical elements.
 * The prover takes nof_mle_polynomials tables of mle_polynomial_size = 2^L elements, a combine function g of that many inputs with
 * polynomial degree d, and the claimed sum; the proof is L round polynomials of d + 1 evaluations at x = 0..d. Round r >= 1 first
 * folds adjacent elements, T_r[j] = T_{r-1}[2j] + alpha_r (T_{r-1}[2j+1] - T_{r-1}[2j]); alpha_0 = 0 is recorded in the challenge
 * vector and never used, alpha_r = F(H(message of round r - 1)) with F the whole digest as one little-endian integer mod p
 * (transcript bytes: INTEGRATION.md). verify: R_0[0] + R_0[1] = claimed_sum, and R_r(alpha_{r+1}) = R_{r+1}[0] + R_{r+1}[1] for
 * r < L - 1; the last round polynomial is not checked against anything, as in the reference. A proof no prover makes (no rounds,
 * round polynomials of different or impossible lengths, a word at or above p) is a wrong proof: *is_verified = false with SUCCESS.
 * Programs: the predefined AB_MINUS_C (id 0: inputs A, B, C, degree 2) and EQ_X_AB_MINUS_C (id 1: A, B, C, E, E (A B - C), degree 3),
 * or a function built from symbols -- input, constant, add, sub, multiply, inverse -- and compiled by
 * <field>_generate_returning_value_program(parameters, nof_parameters, &program): the inputs' symbols followed by the return value's.
 * Symbols belong to the library; every generate call frees all symbols made so far. Degree: input 1, constant 0, add / sub the
 * larger, multiply the sum, inverse -1 (and -1 wherever it is used).
 * <field>_hip_sumcheck_prove is <field>_sumcheck_get_proof writing into a proof made by the caller and returning the error
 * (get_proof returns NULL on any failure). INVALID_ARGUMENT, before the device is touched: mle_polynomial_size no power of two or
 * < 2, nof_mle_polynomials not the program's input count or above 8, degree below 1 or above 6, more than 20 variables (parameters
 * + constants + one per operation; the return value's node takes the output parameter's slot), use_extension_field, a program of
 * another field. NULL pointers: INVALID_POINTER. `batch` is ignored, as the reference ignores it; `stream` is honoured; prove
 * returns with the stream drained (the proof is host data). The caller's polynomials are never written.
 * get_challenge_vector copies min(*size, the vector's length) elements and stores that count in *size.
 * The three serialisation functions, proof_print and the extension_ / rns_ variants are not built. ---- */
typedef struct {
  icicleStreamHandle stream;      /* 0  */
  bool use_extension_field;       /* 8   must be false */
  uint64_t batch;                 /* 16  ignored */
  bool are_inputs_on_device;      /* 24 */
  bool is_async;                  /* 25 */
  icicle_config_extension_t* ext; /* 32 */
} icicle_sumcheck_config_t;
typedef struct {
  icicle_hasher_handle_t hasher;         /* 0  */
  const uint8_t* domain_separator_label; /* 8  */
  size_t domain_separator_label_len;     /* 16 */
  const uint8_t* round_poly_label;       /* 24 */
  size_t round_poly_label_len;           /* 32 */
  const uint8_t* round_challenge_label;  /* 40 */
  size_t round_challenge_label_len;      /* 48 */
  bool little_endian;                    /* 56  carried, unused (as in the reference) */
  const uint32_t* seed_rng;              /* 64  one element of F, canonical */
} icicle_sumcheck_transcript_config_t;
typedef struct icicle_sumcheck* icicle_sumcheck_handle_t;
typedef struct icicle_sumcheck_proof* icicle_sumcheck_proof_handle_t;
typedef struct icicle_program* icicle_program_handle_t;
typedef struct icicle_symbol* icicle_symbol_handle_t;
icicle_error_t delete_program(icicle_program_handle_t program);
#define ICICLE_HIP_DECLARE_SUMCHECK(P)                                                                                 \
  icicle_sumcheck_handle_t P##_sumcheck_create(void);                                                                  \
  icicle_error_t P##_sumcheck_delete(icicle_sumcheck_handle_t sumcheck);                                               \
  icicle_sumcheck_proof_handle_t P##_sumcheck_get_proof(icicle_sumcheck_handle_t sumcheck, const uint32_t* const* mle_polynomials, uint64_t mle_polynomial_size, \
                                                        uint64_t nof_mle_polynomials, const uint32_t* claimed_sum, icicle_program_handle_t combine_function, \
                                                        const icicle_sumcheck_transcript_config_t* transcript_config, const icicle_sumcheck_config_t* sumcheck_config); \
  icicle_error_t P##_hip_sumcheck_prove(icicle_sumcheck_handle_t sumcheck, const uint32_t* const* mle_polynomials, uint64_t mle_polynomial_size, \
                                        uint64_t nof_mle_polynomials, const uint32_t* claimed_sum, icicle_program_handle_t combine_function, \
                                        const icicle_sumcheck_transcript_config_t* transcript_config, const icicle_sumcheck_config_t* sumcheck_config, \
                                        icicle_sumcheck_proof_handle_t proof);                                         \
  icicle_error_t P##_sumcheck_verify(icicle_sumcheck_handle_t sumcheck, icicle_sumcheck_proof_handle_t proof, const uint32_t* claimed_sum, \
                                     const icicle_sumcheck_transcript_config_t* transcript_config, bool* is_verified); \
  icicle_sumcheck_proof_handle_t P##_sumcheck_proof_create(uint32_t** polys, uint64_t nof_polynomials, uint64_t poly_size); \
  icicle_error_t P##_sumcheck_proof_get_poly_sizes(icicle_sumcheck_proof_handle_t proof, uint64_t* poly_size, uint64_t* nof_polys); \
  uint32_t* P##_sumcheck_proof_get_round_poly_at(icicle_sumcheck_proof_handle_t proof, uint64_t index);                \
  icicle_error_t P##_sumcheck_proof_delete(icicle_sumcheck_proof_handle_t proof);                                      \
  icicle_error_t P##_sumcheck_get_challenge_vector(icicle_sumcheck_handle_t sumcheck, uint32_t* challenge_vector, size_t* challenge_vector_size); \
  icicle_error_t P##_sumcheck_get_challenge_size(icicle_sumcheck_handle_t sumcheck, size_t* challenge_size);           \
  icicle_program_handle_t P##_create_predefined_returning_value_program(int pre_def);                                  \
  icicle_error_t P##_generate_returning_value_program(icicle_symbol_handle_t* parameters, int nof_parameters, icicle_program_handle_t* program); \
  icicle_symbol_handle_t P##_create_input_symbol(int in_idx);                                                          \
  icicle_symbol_handle_t P##_create_scalar_symbol(const uint32_t* constant);                                           \
  icicle_symbol_handle_t P##_copy_symbol(icicle_symbol_handle_t other);                                                \
  icicle_error_t P##_add_symbols(icicle_symbol_handle_t op_a, icicle_symbol_handle_t op_b, icicle_symbol_handle_t* res); \
  icicle_error_t P##_sub_symbols(icicle_symbol_handle_t op_a, icicle_symbol_handle_t op_b, icicle_symbol_handle_t* res); \
  icicle_error_t P##_multiply_symbols(icicle_symbol_handle_t op_a, icicle_symbol_handle_t op_b, icicle_symbol_handle_t* res); \
  icicle_error_t P##_inverse_symbol(icicle_symbol_handle_t input, icicle_symbol_handle_t* output);
ICICLE_HIP_DECLARE_SUMCHECK(babybear)
ICICLE_HIP_DECLARE_SUMCHECK(koalabear)
ICICLE_HIP_DECLARE_SUMCHECK(bn254)
ICICLE_HIP_DECLARE_SUMCHECK(bls12_381)
/* backend-specific, for timing tools: while enabled, every prove records device events around each round's two launches; round_times
 * copies the last proof's times (milliseconds, at most `capacity` of them) and stores the number of rounds it has in *rounds */
icicle_error_t icicle_hip_sumcheck_time_rounds(bool enable);
icicle_error_t icicle_hip_sumcheck_round_times(double* ms, int capacity, int* rounds);
/* backend-specific, for tests: a round launch has min(ceil(items / *block), *max_grid) blocks of *block lanes, which walk on over the
 * items beyond; `predefined` non-zero for the predefined programs, 0 for user programs. SumcheckConfig.ext int
 * "hip_sumcheck_max_grid" lowers the cap for one prove (absent or <= 0: *max_grid, larger values are clamped to it). Needs no device. */
icicle_error_t icicle_hip_sumcheck_launch_info(int predefined, int* block, int* max_grid);

/* ---- execute_program: include/icicle/vec_ops.h:404, src/vec_ops.cpp:566, src/program/program_c_api.cpp:35, :48. Over the fields that
 * have the symbol functions above. A program has nof_parameters parameters, each a vector of size * batch_size canonical elements
 * (columns_batch changes nothing: the operation is element-wise); any of them may be read, written or both.
 * <field>_create_predefined_program(pre_def): AB_MINUS_C (id 0: parameters A, B, C and the output A B - C) or EQ_X_AB_MINUS_C (id 1:
 * A, B, C, E and the output E (A B - C)); NULL for any other id. <field>_generate_program(parameters, nof_parameters, &program):
 * parameters[i] is the symbol whose value parameter i has afterwards -- the input symbol i itself for a parameter the program leaves
 * alone. It frees all symbols made so far; delete_program deletes both kinds of program, and execute_program accepts both.
 * Per element: the variables are the parameters' values, then the constants, then the intermediates; the instructions run in the
 * reference's order (parameters in order, each subtree in post-order, operand 1 before operand 2, a COPY where a parameter's node
 * already lives elsewhere); every parameter an instruction wrote is stored back. A parameter read after it was overwritten sees the
 * new value. inverse(0) = 0. One launch per call; a parameter the program does not read is not loaded, one it does not write is not
 * stored, and with host data only those are copied. config->is_a_on_device governs every pointer in data; stream and is_async as
 * in the other vector operations. A pointer may be passed for two parameters (all loads of an element precede its stores);
 * partial overlap is undefined.
 * Before the device is touched: INVALID_POINTER for a NULL program, config, data or data[i]; INVALID_ARGUMENT for nof_params other
 * than the program's, a program of a field of another element size, and a program with more values alive at once, constants
 * included, than the variable file holds: 64 for the one-word fields, 24 for the eight-word ones. size = 0: SUCCESS.
 * The extension_ and rns_ variants and the other fields are not built. ---- */
#define ICICLE_HIP_DECLARE_EXECUTE_PROGRAM(P)                                                                          \
  icicle_program_handle_t P##_create_predefined_program(int pre_def);                                                  \
  icicle_error_t P##_generate_program(icicle_symbol_handle_t* parameters, int nof_parameters, icicle_program_handle_t* program); \
  icicle_error_t P##_execute_program(void** data, uint64_t nof_params, icicle_program_handle_t program, uint64_t size, const icicle_vec_ops_config_t* config);
ICICLE_HIP_DECLARE_EXECUTE_PROGRAM(babybear)
ICICLE_HIP_DECLARE_EXECUTE_PROGRAM(koalabear)
ICICLE_HIP_DECLARE_EXECUTE_PROGRAM(bn254)
ICICLE_HIP_DECLARE_EXECUTE_PROGRAM(bls12_381)

/* ---- backend-specific helpers (not part of the reference ABI) ---- */
const char* icicle_hip_version(void);
/* The window plan msm() would use for this size / config: c = window bits, nwin = number of c-bit windows of a
 * scalar_bits-bit scalar (signed digits, so ceil((scalar_bits + 1) / c)). For operation counts in benchmarks. */
icicle_error_t icicle_hip_msm_plan(int msm_size, int scalar_bits, const icicle_msm_config_t* config, int* c, int* nwin);
/* The whole plan, for tests and benchmarks: out[0..7] = c (bits of the widest windows), nwin, n_lo (number of windows that are one bit
 * narrower -- the mixed-width plans picked from 2^23 terms up), negate (1 = scalars with the top bit set are replaced by r - s and
 * their point negated, icicle/backend/cpu/src/curve/cpu_msm.hpp:276-277), buckets per window slot, buckets in use, segment size,
 * windows per precomputed-table entry. force_windows = MSMConfig.ext "hip_msm_windows" (0: the cost model decides, as msm() does). */
icicle_error_t icicle_hip_msm_plan_info(int msm_size, int scalar_bits, const icicle_msm_config_t* config, int force_windows, int* out);
/* The route <curve>_ecntt would take in this process for size * batch points of point_bytes each in the kernels' form (108: bn254,
 * 168: bls12_381 / bls12_377), for tests: out[0] = number of stages, out[1] = rmax (width of the widest stage; 1 = the radix-2 kernel,
 * more = the matrix form), out[2] = 1 if the radix-2 stages keep their tables in global memory instead of LDS, out[3] = 1 if a scale
 * pass runs (inverse, or coset: a coset generator other than 1), out[4] = 1 if that pass keeps its tables in global memory,
 * out[5 + i] = width of stage i. `out` holds 5 + log2(size) ints. ICICLE_HIP_ECNTT_RADIX_LOG / _QUADS / _GTABS are taken into account. */
icicle_error_t icicle_hip_ecntt_plan_info(int point_bytes, int size, int batch, bool inverse, bool coset, int* out);
/* Device-side synthetic input generator for benchmarks: fills `out` (device or host per flag) with
 * `n` DISTINCT affine points (k0 + i) * G in the reference's canonical affine layout. */
icicle_error_t bn254_hip_generate_affine_points(void* out, int n, uint64_t k0, bool out_on_device, icicleStreamHandle stream);
icicle_error_t bls12_381_hip_generate_affine_points(void* out, int n, uint64_t k0, bool out_on_device, icicleStreamHandle stream);
/* Device-side sum of n projective points (reference layout, device pointers): the combine step of a
 * base-sharded multi-GPU MSM after the RCCL all-gather of per-GPU partial results. */
icicle_error_t bn254_hip_projective_sum(const void* points, int n, void* out, icicleStreamHandle stream);
icicle_error_t bls12_381_hip_projective_sum(const void* points, int n, void* out, icicleStreamHandle stream);
icicle_error_t bn254_g2_hip_generate_affine_points(void* out, int n, uint64_t k0, bool out_on_device, icicleStreamHandle stream);
icicle_error_t bls12_381_g2_hip_generate_affine_points(void* out, int n, uint64_t k0, bool out_on_device, icicleStreamHandle stream);
icicle_error_t bn254_g2_hip_projective_sum(const void* points, int n, void* out, icicleStreamHandle stream);
icicle_error_t bls12_381_g2_hip_projective_sum(const void* points, int n, void* out, icicleStreamHandle stream);
/* data[r][c] *= w_N^(+-(row0+r)*c) on device (N = 2^logn_total, w_N from the initialised domain): the inter-step
 * twiddle of a 4-step NTT whose two steps run on different GPUs (icicle_amd/dist.py, all-to-all over RCCL). */
icicle_error_t babybear_hip_twiddle_rows(uint32_t* data, uint64_t rows, uint64_t cols, uint64_t row0, uint32_t logn_total, bool inverse, icicleStreamHandle stream);
icicle_error_t koalabear_hip_twiddle_rows(uint32_t* data, uint64_t rows, uint64_t cols, uint64_t row0, uint32_t logn_total, bool inverse, icicleStreamHandle stream);
/* Average device time (ms) of the dominant kernel's launches since the last reset, measured with
 * hipEvents on the launch stream (bench.py's live roofline figure). which: 0 = MSM bucket
 * accumulation, 1 = NTT pass kernels, 2 = MSM digit extraction + bucket sort (everything in front of the
 * accumulation), 3 = MSM bucket reduction + window combine (everything behind it). */
icicle_error_t icicle_hip_kernel_timing(int which, bool reset, double* total_ms, int* launches);
icicle_error_t icicle_hip_enable_kernel_timing(bool enable);
/* Roofs of the dominant MSM kernel, measured on the spot (bench.py reports them next to the kernel's own rate):
 * XYZZ mixed additions per second with all operands in registers (curve 0 = bn254, 1 = bls12_381) -- the integer-ALU
 * roof of bucket accumulation -- and random 64-byte gathers per second over a region of `region_bytes` (the access
 * pattern of its base fetch; also the known-byte-count kernel the FETCH_SIZE counter is calibrated on). */
icicle_error_t icicle_hip_ubench_mixed_add(int curve, double* adds_per_second);
icicle_error_t icicle_hip_ubench_gather(uint64_t region_bytes, uint64_t gathers, double* gathers_per_second);
/* VALU-issue roof of the NTT pass kernels, measured on the spot (field 0 = babybear, 1 = koalabear): "pass units" per second, one
 * unit = 16 elements through one 8-stage pass with every operand in registers (two radix-16 register rounds of k_ntt_fast's own
 * butterfly code + the 16 products with the factor behind the pass; no memory, no LDS). A three-pass 2^24-point transform is
 * 3 * 2^20 units per row (reference semantics of the butterflies: icicle/backend/cpu/include/ntt_cpu.h:129-225). */
icicle_error_t icicle_hip_ubench_ntt_pass(int field, double* pass_units_per_second);
/* Device self-test of the in-place asm field products with aliased and constant operands (curve 0 = bn254, 1 = bls12_381):
 * *mismatches must be 0 (tests/test_gpu_msm.py). */
icicle_error_t icicle_hip_selftest_inplace_products(int curve, int* mismatches);
/* Quad-cooperative complete addition / doubling (the ECNTT's butterflies, the MSM's window combine on the GPU) against the one-lane
 * formulas of the reference (projective.h:73-143) on every pair (a G, +- b G), a, b = 0..6 -- P = Q, P = -Q and the identity included --
 * as group elements. curve 0 = bn254, 1 = bls12_381, 2 = bls12_377; *mismatches must come back 0. */
icicle_error_t icicle_hip_selftest_quad_group_ops(int curve, int* mismatches);
/* msm()/ntt() keep their temporaries cached between calls (about 8 GiB after a 2^26-term MSM). release_workspace gives
 * the idle part back to the device (it is also given back automatically when an allocation would otherwise fail, and by
 * <field>_ntt_release_domain); workspace_bytes reports what is cached for the active device. */
icicle_error_t icicle_hip_release_workspace(void);
icicle_error_t icicle_hip_workspace_bytes(size_t* bytes);
/* MSMConfig.ext / NTTConfig.ext keys this backend reads (include/icicle/backend/msm_config.h:4-16 is the reference's
 * vehicle for backend knobs; the plugin copies them out of the reference's ConfigExtension key by key):
 *   "hip_num_devices"          int   msm + ntt: cut the work into this many shards over min(G, visible GPUs) devices
 *   "hip_msm_exchange_buckets" bool  msm: exchange bucket slices (grouped send / recv) instead of partial results
 *   "hip_bases_resident"       bool  msm: keep the per-device copies of the base shards between calls (the caller
 *                                    promises the bases at that pointer do not change); released by the function below --
 *                                    MANDATORY before the address is reused unless the memory came from icicle_malloc
 *                                    (icicle_free releases the copies) --, or versioned with
 *   "hip_bases_generation"     int   msm: caller's content id, part of the cache key (a new value stages fresh copies)
 *   "hip_msm_windows"          int   msm (single MSM, precompute_factor 1, c = 0, full-width scalars): W windows whose widths add up
 *                                    to the scalar bits, the top ones one bit wider, with the reference's negate-if-top-bit-set trick
 *                                    (cpu_msm.hpp:276-277). The cost model picks such a plan by itself from 2^23 terms up (BN254 2^26:
 *                                    10 x 21 + 2 x 22 bits); the key forces one at any size (parity tests, A/B runs)
 *   "hip_msm_passb_own_max"    int   msm (test hook): pass B of the two-level sort lets ONE block sort a whole (window, high key bits)
 *                                    partition of at most this many elements, with its histogram, scan and write cursors in LDS;
 *                                    larger partitions are cut into sub-chunks. 0: no partition is sorted that way; absent: 2^18
 *   "hip_force_rccl"           bool  msm, ntt: take the RCCL exchanges even with one device slot -- all-gather, and the grouped
 *                                    ncclSend / ncclRecv of the bucket exchange and of the split transform as sends to
 *                                    the own rank of a size-1 communicator (test hook: the real librccl on one GPU)
 * icicle_hip_msm_release_resident_bases(bases) frees the resident copies made for `bases` (NULL: for every pointer);
 * icicle_free / icicle_free_async of a device allocation release the copies made for it as well. */
icicle_error_t icicle_hip_msm_release_resident_bases(const void* bases);
/* Counters of what the multi-device / pipelined paths moved since the last reset: { base bytes staged to a device, scalar
 * bytes staged, bytes sent by the bucket exchange / the split transform's all-to-all, resident-base hits (shards NOT staged
 * again), calls that ran one host thread per device slot, point-to-point messages sent, cross-device copies that took the
 * no-peer-access route, MSMs re-run on the uniform window plan after the mixed-width plan did not get its memory }.
 * icicle_hip_multi_stats2 writes the first min(n, 8) of them; icicle_hip_multi_stats writes exactly the first FIVE (out[5], the
 * contract since round 3). */
icicle_error_t icicle_hip_multi_stats(uint64_t* out5, bool reset);
icicle_error_t icicle_hip_multi_stats2(uint64_t* out, int n, bool reset);
/* What the collectives library (RCCL, or the one set with icicle_hip_set_collectives_library) reported for the most recently created
 * communicator set of the in-process multi-GPU path: out[0] ncclGetVersion, out[1] devices asked for, out[2] ncclCommCount,
 * out[3] 1 when every slot p reported ncclCommUserRank == p and ncclCommCount == devices (a set that does not is refused with
 * INVALID_DEVICE), out[4] communicator sets created so far. -1 where the library does not export the call. Writes min(n, 5) values. */
icicle_error_t icicle_hip_collectives_info(int* out, int n);
/* The multi-device paths take their collectives from a library with the NCCL C ABI (ncclCommInitAll, ncclCommDestroy,
 * ncclAllGather, ncclSend, ncclRecv, ncclGroupStart, ncclGroupEnd, ncclGetErrorString), bound with dlopen: librccl.so by default,
 * or the library at `path` (NULL / "" = default again; ICICLE_HIP_RCCL_LIB in the environment does the same) -- another RCCL
 * build, or the in-process stand-in the rehearsal tests build from tests/loopback/ (real RCCL refuses one GPU twice in a
 * communicator). Communicators are cached per library and device list. */
icicle_error_t icicle_hip_set_collectives_library(const char* path);
/* Rehearsal hooks for the multi-device code on a box with fewer GPUs than device slots (tests only): K virtual device slots
 * mapped round-robin onto the physical GPUs, and a one-shot failure of device slot `slot` at stage 1 (worker set-up), 2 (right
 * before the bucket-exchange gate / the split transform's second exchange) or 3 (right before the result-gather gate); stage 0
 * disarms. (slot 0, stage 9): the next single-device msm() "fails to allocate" its first plan once -- the rehearsal of the fallback
 * from the auto-selected mixed-width window plan to the uniform one. */
icicle_error_t icicle_hip_test_set_virtual_devices(int slots);
/* Rehearsal of the case "hipDeviceEnablePeerAccess is refused" (also ICICLE_HIP_NO_PEER_ACCESS=1): the in-process multi-GPU paths then move
 * device-resident operands and results with hipMemcpyPeerAsync (staged through host memory by the HIP runtime when the two devices
 * are not peers) instead of direct hipMemcpyDefault copies. Counted in icicle_hip_multi_stats2's 7th value. */
icicle_error_t icicle_hip_test_set_no_peer_access(bool off);
icicle_error_t icicle_hip_test_inject_failure(int slot, int stage);

/* ---- collision-free aliases used by the reference-runtime plugin (plugin/):
 * same functions as the un-prefixed names above, for processes that also load the reference's own
 * libicicle_device / libicicle_curve_<c> / libicicle_field_<f>, which define those names. ---- */
icicle_error_t icicle_hip_set_device(int device_id);
icicle_config_extension_t* icicle_hip_create_config_extension(void);
void icicle_hip_destroy_config_extension(icicle_config_extension_t* ext);
void icicle_hip_config_extension_set_int(icicle_config_extension_t* ext, const char* key, int value);
void icicle_hip_config_extension_set_bool(icicle_config_extension_t* ext, const char* key, bool value);
icicle_error_t icicle_hip_bn254_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results);
icicle_error_t icicle_hip_bn254_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases);
icicle_error_t icicle_hip_bls12_381_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results);
icicle_error_t icicle_hip_bls12_381_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases);
icicle_error_t icicle_hip_bn254_g2_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results);
icicle_error_t icicle_hip_bn254_g2_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases);
icicle_error_t icicle_hip_bls12_381_g2_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results);
icicle_error_t icicle_hip_bls12_381_g2_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases);
#define ICICLE_HIP_DECLARE_NTT_ALIASES(F)                                                                              \
  icicle_error_t icicle_hip_##F##_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u32_t* config, uint32_t* output); \
  icicle_error_t icicle_hip_##F##_extension_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u32_t* config, uint32_t* output); \
  icicle_error_t icicle_hip_##F##_ntt_init_domain(const uint32_t* primitive_root, const icicle_ntt_init_domain_config_t* config); \
  icicle_error_t icicle_hip_##F##_ntt_release_domain(void);                                                            \
  icicle_error_t icicle_hip_##F##_get_root_of_unity_from_domain(uint64_t logn, uint32_t* rou);
ICICLE_HIP_DECLARE_NTT_ALIASES(babybear)
ICICLE_HIP_DECLARE_NTT_ALIASES(koalabear)
#define ICICLE_HIP_DECLARE_NTT_U256_ALIASES(F)                                                                         \
  icicle_error_t icicle_hip_##F##_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u256_t* config, uint32_t* output); \
  icicle_error_t icicle_hip_##F##_ntt_init_domain(const uint32_t* primitive_root, const icicle_ntt_init_domain_config_t* config); \
  icicle_error_t icicle_hip_##F##_ntt_release_domain(void);                                                            \
  icicle_error_t icicle_hip_##F##_get_root_of_unity_from_domain(uint64_t logn, uint32_t* rou);
ICICLE_HIP_DECLARE_NTT_U256_ALIASES(bn254)
ICICLE_HIP_DECLARE_NTT_U256_ALIASES(bls12_381)
icicle_error_t icicle_hip_bn254_ecntt(const void* input, int size, int dir, const icicle_ntt_config_u256_t* config, void* output);
icicle_error_t icicle_hip_bls12_381_ecntt(const void* input, int size, int dir, const icicle_ntt_config_u256_t* config, void* output);
ICICLE_HIP_DECLARE_CONVERT(icicle_hip_bn254)
ICICLE_HIP_DECLARE_CONVERT(icicle_hip_bls12_381)
ICICLE_HIP_DECLARE_CONVERT(icicle_hip_babybear)
ICICLE_HIP_DECLARE_CONVERT(icicle_hip_koalabear)
icicle_error_t icicle_hip_babybear_extension_scalar_convert_montgomery(const void* input, uint64_t size, bool is_to_montgomery, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_koalabear_extension_scalar_convert_montgomery(const void* input, uint64_t size, bool is_to_montgomery, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_bn254_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_bn254_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_bls12_381_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_bls12_381_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_bn254_g2_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_bn254_g2_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_bls12_381_g2_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_bls12_381_g2_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);

/* ======================================================================================
 * Further curves / fields of the reference that have an MSM or an NTT (icicle/cmake/features.cmake:6,17,19), with the
 * signatures and layouts of the bn254 / bls12_381 symbols above:
 *   bls12_377  MSM on G1 (L = 12) and on G2 over Fq2 = Fq[u]/(u^2 + 5), NTT over its 253-bit scalar field, ECNTT,
 *              Montgomery conversion, element-wise vector ops     (curves/params/bls12_377.h)
 *   grumpkin   MSM on G1 (L = 8; base field = BN254's scalar field, scalars = BN254's base field), Montgomery
 *              conversion, vector ops; the reference gives it no NTT  (curves/params/grumpkin.h)
 *   stark252   NTT + Montgomery conversion + vector ops over the 252-bit Stark field 2^251 + 17*2^192 + 1
 *              (fields/stark_fields/stark252.h; no curve)
 *   goldilocks NTT, extension-field NTT (quadratic extension u^2 = 7: the two components are transformed with the base
 *              field's twiddles), Montgomery conversion (x * 2^64), vector ops over 2^64 - 2^32 + 1
 *              (fields/stark_fields/goldilocks.h; scalar_t = 2 words, so NTTConfig<scalar_t> is the 40-byte struct below)
 * bw6_761 (761-bit base field) and m31 (no NTT in the reference) are not built.
 * ====================================================================================== */
typedef struct {
  icicleStreamHandle stream;      /* 0  */
  uint32_t coset_gen[2];          /* 8   canonical, {1,0} = no coset */
  int32_t batch_size;             /* 16 */
  bool columns_batch;             /* 20 */
  int32_t ordering;               /* 24  icicle_ntt_ordering_t */
  bool are_inputs_on_device;      /* 28 */
  bool are_outputs_on_device;     /* 29 */
  bool is_async;                  /* 30 */
  icicle_config_extension_t* ext; /* 32 */
} icicle_ntt_config_u64_t;
#define ICICLE_HIP_DECLARE_MSM(S)                                                                                      \
  icicle_error_t S##_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results); \
  icicle_error_t S##_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases); \
  icicle_error_t icicle_hip_##S##_msm(const void* scalars, const void* bases, int msm_size, const icicle_msm_config_t* config, void* results); \
  icicle_error_t icicle_hip_##S##_msm_precompute_bases(const void* input_bases, int nof_bases, const icicle_msm_config_t* config, void* output_bases); \
  icicle_error_t S##_hip_generate_affine_points(void* out, int n, uint64_t k0, bool out_on_device, icicleStreamHandle stream); \
  icicle_error_t S##_hip_projective_sum(const void* points, int n, void* out, icicleStreamHandle stream);              \
  icicle_error_t S##_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output); \
  icicle_error_t S##_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output); \
  icicle_error_t icicle_hip_##S##_affine_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output); \
  icicle_error_t icicle_hip_##S##_projective_convert_montgomery(const void* input, uint64_t n, bool is_into, const icicle_vec_ops_config_t* config, void* output);
ICICLE_HIP_DECLARE_MSM(bls12_377)
ICICLE_HIP_DECLARE_MSM(bls12_377_g2)
ICICLE_HIP_DECLARE_MSM(grumpkin)
ICICLE_HIP_DECLARE_NTT_U256(bls12_377)
ICICLE_HIP_DECLARE_NTT_U256(stark252)
ICICLE_HIP_DECLARE_NTT_U256_ALIASES(bls12_377)
ICICLE_HIP_DECLARE_NTT_U256_ALIASES(stark252)
icicle_error_t bls12_377_ecntt(const void* input, int size, int dir, const icicle_ntt_config_u256_t* config, void* output);
icicle_error_t icicle_hip_bls12_377_ecntt(const void* input, int size, int dir, const icicle_ntt_config_u256_t* config, void* output);
ICICLE_HIP_DECLARE_CONVERT(bls12_377)
ICICLE_HIP_DECLARE_CONVERT(grumpkin)
ICICLE_HIP_DECLARE_CONVERT(stark252)
ICICLE_HIP_DECLARE_CONVERT(icicle_hip_bls12_377)
ICICLE_HIP_DECLARE_CONVERT(icicle_hip_grumpkin)
ICICLE_HIP_DECLARE_CONVERT(icicle_hip_stark252)
ICICLE_HIP_DECLARE_VEC_ARITH(bls12_377)
ICICLE_HIP_DECLARE_VEC_ARITH(grumpkin)
ICICLE_HIP_DECLARE_VEC_ARITH(stark252)
ICICLE_HIP_DECLARE_VEC_INV(bls12_377)
ICICLE_HIP_DECLARE_VEC_INV(grumpkin)
ICICLE_HIP_DECLARE_VEC_INV(stark252)
/* goldilocks: elements are 2 u32 words (extension elements 4) */
icicle_error_t goldilocks_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u64_t* config, uint32_t* output);           /* src/ntt.cpp:11 */
icicle_error_t goldilocks_extension_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u64_t* config, uint32_t* output); /* src/ntt.cpp:90 */
icicle_error_t goldilocks_ntt_init_domain(const uint32_t* primitive_root, const icicle_ntt_init_domain_config_t* config);
icicle_error_t goldilocks_ntt_release_domain(void);
icicle_error_t goldilocks_get_root_of_unity(uint64_t max_size, uint32_t* rou);
icicle_error_t goldilocks_get_root_of_unity_from_domain(uint64_t logn, uint32_t* rou);
icicle_error_t icicle_hip_goldilocks_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u64_t* config, uint32_t* output);
icicle_error_t icicle_hip_goldilocks_extension_ntt(const uint32_t* input, int size, int dir, const icicle_ntt_config_u64_t* config, uint32_t* output);
icicle_error_t icicle_hip_goldilocks_ntt_init_domain(const uint32_t* primitive_root, const icicle_ntt_init_domain_config_t* config);
icicle_error_t icicle_hip_goldilocks_ntt_release_domain(void);
icicle_error_t icicle_hip_goldilocks_get_root_of_unity_from_domain(uint64_t logn, uint32_t* rou);
ICICLE_HIP_DECLARE_CONVERT(goldilocks)
ICICLE_HIP_DECLARE_CONVERT(icicle_hip_goldilocks)
icicle_error_t goldilocks_extension_scalar_convert_montgomery(const void* input, uint64_t size, bool is_to_montgomery, const icicle_vec_ops_config_t* config, void* output);
icicle_error_t icicle_hip_goldilocks_extension_scalar_convert_montgomery(const void* input, uint64_t size, bool is_to_montgomery, const icicle_vec_ops_config_t* config, void* output);
ICICLE_HIP_DECLARE_VEC_ARITH(goldilocks)
ICICLE_HIP_DECLARE_VEC_INV(goldilocks)

#ifdef __cplusplus
}
#endif
#endif /* ICICLE_HIP_H */
