"""ctypes binding of libicicle_hip.so (the C ABI declared in include/icicle_hip.h).

The product path has NO CPU fallback: if the HIP library is missing this module raises at import
time; if it is present but there is no GPU every compute entry point returns INVALID_DEVICE.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ICICLE_HIP_LIB", os.path.join(_HERE, "lib", "libicicle_hip.so"))


class IcicleError(RuntimeError):
    NAMES = [
        "SUCCESS", "INVALID_DEVICE", "OUT_OF_MEMORY", "INVALID_POINTER", "ALLOCATION_FAILED",
        "DEALLOCATION_FAILED", "COPY_FAILED", "SYNCHRONIZATION_FAILED", "STREAM_CREATION_FAILED",
        "STREAM_DESTRUCTION_FAILED", "API_NOT_IMPLEMENTED", "INVALID_ARGUMENT",
    ]

    def __init__(self, code, what=""):
        self.code = int(code)
        name = self.NAMES[self.code] if 0 <= self.code < len(self.NAMES) else str(self.code)
        super().__init__(f"eIcicleError::{name} {what}".strip())


def check(code, what=""):
    if code != 0:
        raise IcicleError(code, what)


class Device(ctypes.Structure):
    """icicle::Device (include/icicle/device.h:14-48): 68 bytes, id at offset 64."""
    _fields_ = [("type", ctypes.c_char * 64), ("id", ctypes.c_int)]


class DeviceProperties(ctypes.Structure):
    _fields_ = [("using_host_memory", ctypes.c_bool), ("num_memory_regions", ctypes.c_int),
                ("supports_pinned_memory", ctypes.c_bool)]


class MSMConfig(ctypes.Structure):
    """icicle::MSMConfig (include/icicle/msm.h:21-53), 40 bytes; mirrors the Rust #[repr(C)] struct
    (wrappers/rust/icicle-core/src/msm/mod.rs:13-49)."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("precompute_factor", ctypes.c_int),
        ("c", ctypes.c_int),
        ("bitsize", ctypes.c_int),
        ("batch_size", ctypes.c_int),
        ("are_points_shared_in_batch", ctypes.c_bool),
        ("are_scalars_on_device", ctypes.c_bool),
        ("are_scalars_montgomery_form", ctypes.c_bool),
        ("are_points_on_device", ctypes.c_bool),
        ("are_points_montgomery_form", ctypes.c_bool),
        ("are_results_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        # default_msm_config() (msm.h:60-78)
        return cls(None, 1, 0, 0, 1, True, False, False, False, False, False, False, None)


class NTTConfigU32(ctypes.Structure):
    """icicle::NTTConfig<S> for a 4-byte S (include/icicle/ntt.h:53-64), 40 bytes."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("coset_gen", ctypes.c_uint32),
        ("batch_size", ctypes.c_int),
        ("columns_batch", ctypes.c_bool),
        ("ordering", ctypes.c_int),
        ("are_inputs_on_device", ctypes.c_bool),
        ("are_outputs_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        # default_ntt_config() (ntt.h:72-85)
        return cls(None, 1, 1, False, 0, False, False, False, None)


class NTTConfigU256(ctypes.Structure):
    """icicle::NTTConfig<S> for the curves' 32-byte scalar_t (include/icicle/ntt.h:53-64), 64 bytes."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("coset_gen", ctypes.c_uint32 * 8),
        ("batch_size", ctypes.c_int),
        ("columns_batch", ctypes.c_bool),
        ("ordering", ctypes.c_int),
        ("are_inputs_on_device", ctypes.c_bool),
        ("are_outputs_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        one = (ctypes.c_uint32 * 8)(1, 0, 0, 0, 0, 0, 0, 0)
        return cls(None, one, 1, False, 0, False, False, False, None)

    def set_coset_gen(self, g: int):
        for i in range(8):
            self.coset_gen[i] = (g >> (32 * i)) & 0xFFFFFFFF


class NTTConfigU64(ctypes.Structure):
    """icicle::NTTConfig<S> for goldilocks' 8-byte scalar_t, 40 bytes (include/icicle_hip.h icicle_ntt_config_u64_t)."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("coset_gen", ctypes.c_uint32 * 2),
        ("batch_size", ctypes.c_int),
        ("columns_batch", ctypes.c_bool),
        ("ordering", ctypes.c_int),
        ("are_inputs_on_device", ctypes.c_bool),
        ("are_outputs_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        return cls(None, (ctypes.c_uint32 * 2)(1, 0), 1, False, 0, False, False, False, None)

    def set_coset_gen(self, g: int):
        self.coset_gen[0], self.coset_gen[1] = g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF


class VecOpsConfig(ctypes.Structure):
    """icicle::VecOpsConfig (include/icicle/vec_ops.h:19-37), 32 bytes."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("is_a_on_device", ctypes.c_bool),
        ("is_b_on_device", ctypes.c_bool),
        ("is_result_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("batch_size", ctypes.c_int),
        ("columns_batch", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        return cls(None, False, False, False, False, 1, False, None)


class NTTInitDomainConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]

    @classmethod
    def default(cls):
        return cls(None, False, None)


class HashConfig(ctypes.Structure):
    """icicle::HashConfig (include/icicle/hash/hash_config.h:15-24), 32 bytes."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("batch", ctypes.c_uint64),
        ("are_inputs_on_device", ctypes.c_bool),
        ("are_outputs_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        return cls(None, 1, False, False, False, None)


class MerkleTreeConfig(ctypes.Structure):
    """icicle::MerkleTreeConfig (include/icicle/merkle/merkle_tree_config.h:26-37), 24 bytes."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("is_leaves_on_device", ctypes.c_bool),
        ("is_tree_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("padding_policy", ctypes.c_int),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        return cls(None, False, False, False, 0, None)


class PowConfig(ctypes.Structure):
    """icicle::PowConfig (include/icicle/hash/pow.h:16-25), 32 bytes."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("is_challenge_on_device", ctypes.c_bool),
        ("padding_size", ctypes.c_uint32),
        ("is_async", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        # default_pow_config() (pow.h:32)
        return cls(None, False, 24, False, None)


class FriConfig(ctypes.Structure):
    """icicle::FriConfig (include/icicle/fri/fri_config.h:16-25), 56 bytes."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("folding_factor", ctypes.c_size_t),
        ("stopping_degree", ctypes.c_size_t),
        ("pow_bits", ctypes.c_size_t),
        ("nof_queries", ctypes.c_size_t),
        ("are_inputs_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        # default_fri_config() (fri_config.h:35)
        return cls(None, 2, 0, 16, 100, False, False, None)


class FFIFriTranscriptConfig(ctypes.Structure):
    """FFIFriTranscriptConfig (src/fri/fri_c_api.cpp:13-32), 96 bytes; built by icicle_amd.fri.FriTranscriptConfig."""
    _fields_ = [
        ("hasher", ctypes.c_void_p),
        ("domain_separator_label", ctypes.c_void_p), ("domain_separator_label_len", ctypes.c_size_t),
        ("round_challenge_label", ctypes.c_void_p), ("round_challenge_label_len", ctypes.c_size_t),
        ("commit_phase_label", ctypes.c_void_p), ("commit_phase_label_len", ctypes.c_size_t),
        ("nonce_label", ctypes.c_void_p), ("nonce_label_len", ctypes.c_size_t),
        ("public_state", ctypes.c_void_p), ("public_state_len", ctypes.c_size_t),
        ("seed_rng", ctypes.c_void_p),
    ]


class SumcheckConfig(ctypes.Structure):
    """icicle::SumcheckConfig (include/icicle/sumcheck/sumcheck_config.h), 40 bytes."""
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("use_extension_field", ctypes.c_bool),
        ("batch", ctypes.c_uint64),
        ("are_inputs_on_device", ctypes.c_bool),
        ("is_async", ctypes.c_bool),
        ("ext", ctypes.c_void_p),
    ]

    @classmethod
    def default(cls):
        # default_sumcheck_config()
        return cls(None, False, 1, False, False, None)


class FFISumcheckTranscriptConfig(ctypes.Structure):
    """TranscriptConfigFFI (src/sumcheck/sumcheck_c_api.cpp:14-24), 72 bytes; built by icicle_amd.sumcheck.SumcheckTranscriptConfig."""
    _fields_ = [
        ("hasher", ctypes.c_void_p),
        ("domain_separator_label", ctypes.c_void_p), ("domain_separator_label_len", ctypes.c_size_t),
        ("round_poly_label", ctypes.c_void_p), ("round_poly_label_len", ctypes.c_size_t),
        ("round_challenge_label", ctypes.c_void_p), ("round_challenge_label_len", ctypes.c_size_t),
        ("little_endian", ctypes.c_bool),
        ("seed_rng", ctypes.c_void_p),
    ]


assert ctypes.sizeof(Device) == 68 and Device.id.offset == 64
assert ctypes.sizeof(SumcheckConfig) == 40 and [getattr(SumcheckConfig, f).offset for f, _ in SumcheckConfig._fields_] == [0, 8, 16, 24, 25, 32]
assert ctypes.sizeof(FFISumcheckTranscriptConfig) == 72 and FFISumcheckTranscriptConfig.little_endian.offset == 56 and FFISumcheckTranscriptConfig.seed_rng.offset == 64
assert ctypes.sizeof(FriConfig) == 56 and [getattr(FriConfig, f).offset for f, _ in FriConfig._fields_] == [0, 8, 16, 24, 32, 40, 41, 48]
assert ctypes.sizeof(FFIFriTranscriptConfig) == 96 and FFIFriTranscriptConfig.seed_rng.offset == 88
assert ctypes.sizeof(PowConfig) == 32 and [getattr(PowConfig, f).offset for f, _ in PowConfig._fields_] == [0, 8, 12, 16, 24]
assert ctypes.sizeof(HashConfig) == 32 and HashConfig.are_inputs_on_device.offset == 16 and HashConfig.ext.offset == 24
assert ctypes.sizeof(MerkleTreeConfig) == 24 and MerkleTreeConfig.padding_policy.offset == 12 and MerkleTreeConfig.ext.offset == 16
assert ctypes.sizeof(MSMConfig) == 40 and MSMConfig.ext.offset == 32
assert ctypes.sizeof(NTTConfigU32) == 40 and NTTConfigU32.ordering.offset == 20
assert ctypes.sizeof(NTTInitDomainConfig) == 24
assert ctypes.sizeof(NTTConfigU256) == 64 and NTTConfigU256.batch_size.offset == 40 and NTTConfigU256.ordering.offset == 48
assert NTTConfigU256.ext.offset == 56
assert ctypes.sizeof(VecOpsConfig) == 32 and VecOpsConfig.batch_size.offset == 12 and VecOpsConfig.ext.offset == 24

# every symbol include/icicle_hip.h declares (tests/test_abi.py checks the header against this)
RUNTIME_SYMBOLS = [
    "icicle_load_backend", "icicle_load_backend_from_env_or_default", "icicle_set_device",
    "icicle_set_default_device", "icicle_get_active_device", "icicle_is_host_memory",
    "icicle_is_active_device_memory", "icicle_get_device_count", "icicle_malloc", "icicle_malloc_async",
    "icicle_free", "icicle_free_async", "icicle_get_available_memory", "icicle_memset",
    "icicle_memset_async", "icicle_copy", "icicle_copy_async", "icicle_copy_to_host",
    "icicle_copy_to_host_async", "icicle_copy_to_device", "icicle_copy_to_device_async",
    "icicle_create_stream", "icicle_destroy_stream", "icicle_stream_synchronize",
    "icicle_device_synchronize", "icicle_get_device_properties", "icicle_is_device_available",
    "icicle_get_registered_devices",
    "create_config_extension", "destroy_config_extension", "config_extension_set_int",
    "config_extension_set_bool", "config_extension_get_int", "config_extension_get_bool",
    "clone_config_extension",
]
CURVES = ["bn254", "bls12_381", "bls12_377", "grumpkin"]  # G1 MSM
G2_CURVES = ["bn254", "bls12_381", "bls12_377"]
ECNTT_CURVES = ["bn254", "bls12_381", "bls12_377"]
NTT_FIELDS = ["babybear", "koalabear"]
SCALAR_NTT_FIELDS = ["bn254", "bls12_381", "bls12_377", "stark252"]  # NTT over a 256-bit field, 8-word elements
BIG_VEC_FIELDS = SCALAR_NTT_FIELDS + ["grumpkin"]  # element-wise ops / Montgomery conversion over 8-word scalars
GOLD = "goldilocks"  # 2-word elements, NTTConfigU64; extension field = 2 components
# FRI (src/fri/fri_c_api.cpp): the functions that return an error code, per field and again with the prefix <field>_extension
FRI_PREFIXES = [f"{f}{e}" for f in NTT_FIELDS for e in ("", "_extension")]
# the same functions over the wider fields (fri_wide.hip): prefix -> uint32 words of one element
FRI_WIDE_WORDS = {GOLD: 2, f"{GOLD}_extension": 4, "stark252": 8, "bn254": 8, "bls12_381": 8, "bls12_377": 8}
FRI_WIDE_PREFIXES = list(FRI_WIDE_WORDS)
FRI_FUNCTIONS = ["icicle_delete_fri_proof", "fri_proof_get_nof_queries", "fri_proof_get_nof_rounds", "fri_proof_get_round_proofs_for_query",
                 "fri_proof_get_final_poly_size", "fri_proof_get_final_poly", "fri_proof_get_pow_nonce", "fri_merkle_tree_prove", "fri_merkle_tree_verify",
                 "hip_fri_fold"]
# Sumcheck, programs and symbols (src/sumcheck/sumcheck_c_api.cpp, src/program/program_c_api.cpp, src/symbol/symbol_api.cpp): the
# functions that return an error code, per field; words of an element per field
SUMCHECK_FIELDS = {"babybear": 1, "koalabear": 1, "bn254": 8, "bls12_381": 8}
SUMCHECK_FUNCTIONS = ["sumcheck_delete", "hip_sumcheck_prove", "sumcheck_verify", "sumcheck_proof_get_poly_sizes", "sumcheck_proof_delete",
                      "sumcheck_get_challenge_vector", "sumcheck_get_challenge_size", "generate_returning_value_program", "add_symbols", "sub_symbols",
                      "multiply_symbols", "inverse_symbol"]
# execute_program and the general program (src/vec_ops.cpp:566, src/program/program_c_api.cpp:48): the functions that return an error code
PROGRAM_FUNCTIONS = ["generate_program", "execute_program"]
# the extension-field vector operations (src/vec_ops.cpp:24-464, EXT_FIELD), for NTT_FIELDS + [GOLD]: two operands, one operand
EXT_VEC_OPS_2 = ["vector_add", "vector_sub", "vector_mul", "vector_div", "vector_mixed_mul", "scalar_add_vec", "scalar_sub_vec", "scalar_mul_vec"]
EXT_VEC_OPS_1 = ["vector_inv", "vector_sum", "vector_product", "bit_reverse"]
# slice, highest_non_zero_idx, poly_eval, poly_division (src/vec_ops.cpp:472-677), for NTT_FIELDS + BIG_VEC_FIELDS + [GOLD]
POLY_OPS = ["slice", "highest_non_zero_idx", "poly_eval", "poly_division"]
API_SYMBOLS = (
    [f"{c}_{s}" for c in CURVES for s in ("msm", "msm_precompute_bases", "hip_generate_affine_points", "hip_projective_sum")]
    + [f"{c}_g2_{s}" for c in G2_CURVES for s in ("msm", "msm_precompute_bases", "hip_generate_affine_points", "hip_projective_sum")]
    + [f"icicle_hip_{c}_g2_{s}" for c in G2_CURVES for s in ("msm", "msm_precompute_bases")]
    + [f"{f}_{s}" for f in NTT_FIELDS for s in ("ntt", "ntt_init_domain", "ntt_release_domain", "get_root_of_unity",
                                               "get_root_of_unity_from_domain", "extension_ntt", "hip_twiddle_rows")]
    + [f"{f}_{s}" for f in SCALAR_NTT_FIELDS for s in ("ntt", "ntt_init_domain", "ntt_release_domain", "get_root_of_unity",
                                                      "get_root_of_unity_from_domain")]
    + [f"icicle_hip_{f}_{s}" for f in SCALAR_NTT_FIELDS for s in ("ntt", "ntt_init_domain", "ntt_release_domain",
                                                                 "get_root_of_unity_from_domain")]
    + [f"{pre}{c}_ecntt" for pre in ("", "icicle_hip_") for c in ECNTT_CURVES]
    + [f"{GOLD}_{s}" for s in ("ntt", "extension_ntt", "ntt_init_domain", "ntt_release_domain", "get_root_of_unity", "get_root_of_unity_from_domain")]
    + [f"icicle_hip_{GOLD}_{s}" for s in ("ntt", "extension_ntt", "ntt_init_domain", "ntt_release_domain", "get_root_of_unity_from_domain")]
    + [f"{pre}{f}_{op}" for pre in ("", "icicle_hip_") for f in NTT_FIELDS + BIG_VEC_FIELDS + [GOLD]
       for op in ("vector_add", "vector_sub", "vector_mul", "scalar_mul_vec", "scalar_add_vec", "scalar_sub_vec", "bit_reverse")]
    + [f"{f}_{op}" for f in NTT_FIELDS + BIG_VEC_FIELDS + [GOLD] for op in ("vector_inv", "vector_div", "vector_sum", "vector_product")]
    + ["icicle_hip_vector_inv_tile"]
    + [f"{f}_{op}" for f in NTT_FIELDS + BIG_VEC_FIELDS + [GOLD] for op in POLY_OPS]
    + ["icicle_hip_poly_division_tile"]
    + [f"{f}_extension_{op}" for f in NTT_FIELDS + [GOLD] for op in EXT_VEC_OPS_2 + EXT_VEC_OPS_1] + ["icicle_hip_extension_vector_inv_tile"]
    + [f"{pre}{f}_matrix_transpose" for pre in ("", "icicle_hip_") for f in NTT_FIELDS + BIG_VEC_FIELDS + [GOLD]]
    + [f"{pre}{f}_extension_matrix_transpose" for pre in ("", "icicle_hip_") for f in NTT_FIELDS + [GOLD]]
    + ["icicle_hip_msm_plan", "icicle_hip_msm_plan_info", "icicle_hip_ecntt_plan_info", "icicle_hip_version", "icicle_hip_kernel_timing", "icicle_hip_enable_kernel_timing", "icicle_hip_set_device",
       "icicle_hip_ubench_mixed_add", "icicle_hip_ubench_gather", "icicle_hip_ubench_ntt_pass", "icicle_hip_selftest_inplace_products", "icicle_hip_selftest_quad_group_ops", "icicle_hip_release_workspace", "icicle_hip_workspace_bytes",
       "icicle_hip_msm_release_resident_bases", "icicle_hip_multi_stats", "icicle_hip_multi_stats2", "icicle_hip_collectives_info", "icicle_hip_test_set_virtual_devices", "icicle_hip_test_set_no_peer_access",
       "icicle_hip_set_collectives_library", "icicle_hip_test_inject_failure",
       "icicle_hip_create_config_extension", "icicle_hip_destroy_config_extension", "icicle_hip_config_extension_set_int",
       "icicle_hip_config_extension_set_bool"]
    + [f"icicle_hip_{c}_{s}" for c in CURVES for s in ("msm", "msm_precompute_bases")]
    + [f"icicle_hip_{f}_{s}" for f in NTT_FIELDS for s in ("ntt", "extension_ntt", "ntt_init_domain", "ntt_release_domain",
                                                          "get_root_of_unity_from_domain")]
    + [f"{pre}{f}_scalar_convert_montgomery" for pre in ("", "icicle_hip_") for f in BIG_VEC_FIELDS + NTT_FIELDS + [GOLD]]
    + [f"{pre}{f}_extension_scalar_convert_montgomery" for pre in ("", "icicle_hip_") for f in NTT_FIELDS + [GOLD]]
    + [f"{pre}{c}_{k}_convert_montgomery" for pre in ("", "icicle_hip_") for c in CURVES for k in ("affine", "projective")]
    + [f"{pre}{c}_g2_{k}_convert_montgomery" for pre in ("", "icicle_hip_") for c in G2_CURVES for k in ("affine", "projective")]
    + ["icicle_hasher_hash", "icicle_hasher_delete", "icicle_merkle_tree_delete", "icicle_merkle_tree_build", "icicle_merkle_tree_get_proof",
       "icicle_merkle_tree_verify", "icicle_merkle_proof_delete", "icicle_merkle_proof_is_pruned"]
    + ["icicle_hip_merkle_tree_get_proofs", "icicle_hip_merkle_tree_verify_batch"]
    + ["proof_of_work", "proof_of_work_verify"]
    + [f"{p}_{s}" for p in FRI_PREFIXES + FRI_WIDE_PREFIXES for s in FRI_FUNCTIONS]
    + [f"{p}_{s}" for p in SUMCHECK_FIELDS for s in SUMCHECK_FUNCTIONS] + ["delete_program", "icicle_hip_sumcheck_time_rounds", "icicle_hip_sumcheck_round_times",
                                                                         "icicle_hip_sumcheck_launch_info"]
    + [f"{p}_{s}" for p in SUMCHECK_FIELDS for s in PROGRAM_FUNCTIONS]
)
# hash / Merkle functions that return a handle, a size or a byte pointer (tests/test_abi.py's header scan sees only the return types
# of the lists above; tests/test_hash_cpu.py checks these against the header with a scan of its own): name -> restype
_HASH_RESTYPES = {
    "icicle_create_keccak_256": ctypes.c_void_p, "icicle_create_keccak_512": ctypes.c_void_p,
    "icicle_create_sha3_256": ctypes.c_void_p, "icicle_create_sha3_512": ctypes.c_void_p,
    "icicle_hasher_output_size": ctypes.c_uint64,
    "icicle_merkle_tree_create": ctypes.c_void_p, "icicle_merkle_tree_get_root": ctypes.c_void_p,
    "icicle_merkle_proof_create": ctypes.c_void_p, "icicle_merkle_proof_create_with_data": ctypes.c_void_p,
    "icicle_merkle_proof_get_path": ctypes.c_void_p, "icicle_merkle_proof_get_leaf": ctypes.c_void_p,
    "icicle_merkle_proof_get_root": ctypes.c_void_p,
}
HASH_HANDLE_SYMBOLS = list(_HASH_RESTYPES)
# the Blake factories (hash_c_api.cpp:123, :136), a table of their own: name -> restype
BLAKE_HANDLE_SYMBOLS = {"icicle_create_blake2s": ctypes.c_void_p, "icicle_create_blake3": ctypes.c_void_p}
# the Poseidon2 factories (poseidon2_c_api.cpp:13), per field: name -> restype
POSEIDON2_FIELDS = ["babybear", "koalabear"]
POSEIDON2_HANDLE_SYMBOLS = {f"{f}_create_poseidon2_hasher": ctypes.c_void_p for f in POSEIDON2_FIELDS}
# the same entry over the 256-bit fields (elements of 32 bytes, widths 2, 3, 4, 8): a list of its own, POSEIDON2_FIELDS means 4-byte elements
POSEIDON2_WIDE_FIELDS = ["bn254", "bls12_381", "bls12_377", "grumpkin", "stark252"]
POSEIDON2_WIDE_HANDLE_SYMBOLS = {f"{f}_create_poseidon2_hasher": ctypes.c_void_p for f in POSEIDON2_WIDE_FIELDS}
# and over Goldilocks (elements of 8 bytes, the eight widths of the 31-bit fields): again a list of its own
POSEIDON2_GOLD_FIELDS = ["goldilocks"]
POSEIDON2_GOLD_HANDLE_SYMBOLS = {f"{f}_create_poseidon2_hasher": ctypes.c_void_p for f in POSEIDON2_GOLD_FIELDS}
# the Poseidon factories (poseidon_c_api.cpp), per scalar field: name -> restype
POSEIDON_FIELDS = ["bn254", "bls12_381", "bls12_377", "grumpkin"]
POSEIDON_HANDLE_SYMBOLS = {f"{f}_create_poseidon_hasher": ctypes.c_void_p for f in POSEIDON_FIELDS}
# the two FRI functions that return a proof handle: name -> restype
FRI_HANDLE_SYMBOLS = {f"{p}_{s}": ctypes.c_void_p for p in FRI_PREFIXES + FRI_WIDE_PREFIXES for s in ("icicle_initialize_fri_proof", "icicle_create_with_arguments_fri_proof")}
# the sumcheck, program and symbol functions that return a handle or a pointer: name -> restype
SUMCHECK_HANDLE_SYMBOLS = {f"{p}_{s}": ctypes.c_void_p for p in SUMCHECK_FIELDS
                           for s in ("sumcheck_create", "sumcheck_get_proof", "sumcheck_proof_create", "sumcheck_proof_get_round_poly_at",
                                     "create_predefined_returning_value_program", "create_input_symbol", "create_scalar_symbol", "copy_symbol")}
# program_c_api.cpp:35: name -> restype
PROGRAM_HANDLE_SYMBOLS = {f"{p}_create_predefined_program": ctypes.c_void_p for p in SUMCHECK_FIELDS}

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). icicle_amd has no CPU fallback."
    )
lib = ctypes.CDLL(LIB_PATH)
for _s in RUNTIME_SYMBOLS + API_SYMBOLS:
    getattr(lib, _s)  # AttributeError if the library does not export a declared symbol
for _s in HASH_HANDLE_SYMBOLS:
    getattr(lib, _s).restype = _HASH_RESTYPES[_s]  # AttributeError if the symbol is missing, as above
for _s, _r in BLAKE_HANDLE_SYMBOLS.items():
    getattr(lib, _s).restype = _r
    getattr(lib, _s).argtypes = [ctypes.c_uint64]
lib.icicle_hip_version.restype = ctypes.c_char_p
lib.create_config_extension.restype = ctypes.c_void_p
lib.clone_config_extension.restype = ctypes.c_void_p
lib.clone_config_extension.argtypes = [ctypes.c_void_p]
lib.destroy_config_extension.argtypes = [ctypes.c_void_p]
lib.config_extension_set_int.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
lib.config_extension_set_bool.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_bool]
lib.config_extension_get_int.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
lib.config_extension_get_bool.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
lib.config_extension_get_bool.restype = ctypes.c_bool
for _n in ("icicle_malloc",):
    getattr(lib, _n).argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
lib.icicle_malloc_async.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_void_p]
lib.icicle_free.argtypes = [ctypes.c_void_p]
lib.icicle_free_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.icicle_memset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
lib.icicle_memset_async.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
for _n in ("icicle_copy", "icicle_copy_to_host", "icicle_copy_to_device"):
    getattr(lib, _n).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
for _n in ("icicle_copy_async", "icicle_copy_to_host_async", "icicle_copy_to_device_async"):
    getattr(lib, _n).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
lib.icicle_is_host_memory.argtypes = [ctypes.c_void_p]
lib.icicle_is_active_device_memory.argtypes = [ctypes.c_void_p]
lib.icicle_create_stream.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
lib.icicle_destroy_stream.argtypes = [ctypes.c_void_p]
lib.icicle_stream_synchronize.argtypes = [ctypes.c_void_p]
lib.icicle_get_available_memory.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
lib.icicle_get_registered_devices.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
for _c in CURVES:
    getattr(lib, f"{_c}_msm").argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(MSMConfig), ctypes.c_void_p]
    getattr(lib, f"{_c}_msm_precompute_bases").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(MSMConfig), ctypes.c_void_p]
    getattr(lib, f"{_c}_hip_projective_sum").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    getattr(lib, f"{_c}_hip_generate_affine_points").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_bool, ctypes.c_void_p]
for _c in G2_CURVES:
    getattr(lib, f"{_c}_g2_msm").argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(MSMConfig), ctypes.c_void_p]
    getattr(lib, f"{_c}_g2_msm_precompute_bases").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(MSMConfig), ctypes.c_void_p]
    getattr(lib, f"{_c}_g2_hip_projective_sum").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    getattr(lib, f"{_c}_g2_hip_generate_affine_points").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_bool, ctypes.c_void_p]
for _f in NTT_FIELDS:
    getattr(lib, f"{_f}_ntt").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(NTTConfigU32), ctypes.c_void_p]
    getattr(lib, f"{_f}_extension_ntt").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(NTTConfigU32), ctypes.c_void_p]
    getattr(lib, f"{_f}_ntt_init_domain").argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(NTTInitDomainConfig)]
    getattr(lib, f"{_f}_hip_twiddle_rows").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_bool, ctypes.c_void_p]
    getattr(lib, f"{_f}_get_root_of_unity").argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
    getattr(lib, f"{_f}_get_root_of_unity_from_domain").argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
for _f in ECNTT_CURVES:
    getattr(lib, f"{_f}_ecntt").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(NTTConfigU256), ctypes.c_void_p]
for _f in SCALAR_NTT_FIELDS:
    getattr(lib, f"{_f}_ntt").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(NTTConfigU256), ctypes.c_void_p]
    getattr(lib, f"{_f}_ntt_init_domain").argtypes = [ctypes.c_void_p, ctypes.POINTER(NTTInitDomainConfig)]
    getattr(lib, f"{_f}_get_root_of_unity").argtypes = [ctypes.c_uint64, ctypes.c_void_p]
    getattr(lib, f"{_f}_get_root_of_unity_from_domain").argtypes = [ctypes.c_uint64, ctypes.c_void_p]
for _s in ("ntt", "extension_ntt"):
    getattr(lib, f"{GOLD}_{_s}").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(NTTConfigU64), ctypes.c_void_p]
getattr(lib, f"{GOLD}_ntt_init_domain").argtypes = [ctypes.c_void_p, ctypes.POINTER(NTTInitDomainConfig)]
getattr(lib, f"{GOLD}_get_root_of_unity").argtypes = [ctypes.c_uint64, ctypes.c_void_p]
getattr(lib, f"{GOLD}_get_root_of_unity_from_domain").argtypes = [ctypes.c_uint64, ctypes.c_void_p]
for _f in NTT_FIELDS + BIG_VEC_FIELDS + [GOLD]:
    for _op in ("vector_add", "vector_sub", "vector_mul", "scalar_mul_vec", "scalar_add_vec", "scalar_sub_vec"):
        getattr(lib, f"{_f}_{_op}").argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
    getattr(lib, f"{_f}_bit_reverse").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
    for _op in ("vector_inv", "vector_sum", "vector_product"):
        getattr(lib, f"{_f}_{_op}").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
    getattr(lib, f"{_f}_vector_div").argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
lib.icicle_hip_vector_inv_tile.argtypes = [ctypes.c_int]
_slice_args = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
for _f in NTT_FIELDS + BIG_VEC_FIELDS + [GOLD]:
    getattr(lib, f"{_f}_slice").argtypes = _slice_args
    getattr(lib, f"{_f}_highest_non_zero_idx").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
    getattr(lib, f"{_f}_poly_eval").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
    getattr(lib, f"{_f}_poly_division").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p,
                                                    ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
lib.icicle_hip_poly_division_tile.argtypes = [ctypes.c_int]
for _f in NTT_FIELDS + [GOLD]:
    for _op in EXT_VEC_OPS_2:
        getattr(lib, f"{_f}_extension_{_op}").argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
    for _op in EXT_VEC_OPS_1:
        getattr(lib, f"{_f}_extension_{_op}").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
lib.icicle_hip_extension_vector_inv_tile.argtypes = [ctypes.c_int]
for _n in API_SYMBOLS:
    if _n.endswith("matrix_transpose"):
        getattr(lib, _n).argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
    if _n.endswith("convert_montgomery"):
        getattr(lib, _n).argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_bool, ctypes.POINTER(VecOpsConfig), ctypes.c_void_p]
lib.icicle_hip_kernel_timing.argtypes = [ctypes.c_int, ctypes.c_bool, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
lib.icicle_hip_enable_kernel_timing.argtypes = [ctypes.c_bool]
lib.icicle_hip_msm_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(MSMConfig), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
lib.icicle_hip_msm_plan_info.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(MSMConfig), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
lib.icicle_hip_ecntt_plan_info.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_bool, ctypes.c_bool, ctypes.POINTER(ctypes.c_int)]
lib.icicle_hip_ubench_mixed_add.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
lib.icicle_hip_ubench_ntt_pass.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
lib.icicle_hip_ubench_gather.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)]
lib.icicle_hip_workspace_bytes.argtypes = [ctypes.POINTER(ctypes.c_size_t)]
lib.icicle_hip_selftest_inplace_products.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
lib.icicle_hip_selftest_quad_group_ops.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
lib.icicle_hip_msm_release_resident_bases.argtypes = [ctypes.c_void_p]
lib.icicle_hip_multi_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_bool]
lib.icicle_hip_multi_stats2.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_bool]
lib.icicle_hip_test_set_virtual_devices.argtypes = [ctypes.c_int]
lib.icicle_hip_set_collectives_library.argtypes = [ctypes.c_char_p]
lib.icicle_hip_test_inject_failure.argtypes = [ctypes.c_int, ctypes.c_int]
_size_p = ctypes.POINTER(ctypes.c_size_t)
for _n in ("icicle_create_keccak_256", "icicle_create_keccak_512", "icicle_create_sha3_256", "icicle_create_sha3_512"):
    getattr(lib, _n).argtypes = [ctypes.c_uint64]
for _s, _r in {**POSEIDON2_HANDLE_SYMBOLS, **POSEIDON2_WIDE_HANDLE_SYMBOLS, **POSEIDON2_GOLD_HANDLE_SYMBOLS, **POSEIDON_HANDLE_SYMBOLS}.items():
    getattr(lib, _s).restype = _r
    getattr(lib, _s).argtypes = [ctypes.c_uint, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint]
lib.icicle_hasher_hash.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HashConfig), ctypes.c_void_p]
lib.icicle_hasher_output_size.argtypes = [ctypes.c_void_p]
lib.icicle_hasher_delete.argtypes = [ctypes.c_void_p]
lib.icicle_merkle_tree_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64]
lib.icicle_merkle_tree_delete.argtypes = [ctypes.c_void_p]
lib.icicle_merkle_tree_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(MerkleTreeConfig)]
lib.icicle_merkle_tree_get_root.argtypes = [ctypes.c_void_p, _size_p]
lib.icicle_merkle_tree_get_proof.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_bool,
                                             ctypes.POINTER(MerkleTreeConfig), ctypes.c_void_p]
lib.icicle_merkle_tree_verify.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_bool)]
lib.icicle_hip_merkle_tree_get_proofs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64, ctypes.c_bool,
                                                  ctypes.POINTER(MerkleTreeConfig), ctypes.POINTER(ctypes.c_void_p)]
lib.icicle_hip_merkle_tree_verify_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint64, ctypes.POINTER(ctypes.c_bool)]
lib.icicle_merkle_proof_create.argtypes = []
lib.icicle_merkle_proof_create_with_data.argtypes = [ctypes.c_bool, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                     ctypes.c_void_p, ctypes.c_size_t]
lib.icicle_merkle_proof_delete.argtypes = [ctypes.c_void_p]
lib.icicle_merkle_proof_is_pruned.argtypes = [ctypes.c_void_p]
lib.icicle_merkle_proof_is_pruned.restype = ctypes.c_bool
lib.icicle_merkle_proof_get_path.argtypes = [ctypes.c_void_p, _size_p]
lib.icicle_merkle_proof_get_leaf.argtypes = [ctypes.c_void_p, _size_p, ctypes.POINTER(ctypes.c_uint64)]
lib.icicle_merkle_proof_get_root.argtypes = [ctypes.c_void_p, _size_p]
_u64_p = ctypes.POINTER(ctypes.c_uint64)
lib.proof_of_work.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint8, ctypes.POINTER(PowConfig), ctypes.POINTER(ctypes.c_bool), _u64_p, _u64_p]
lib.proof_of_work_verify.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint8, ctypes.POINTER(PowConfig), ctypes.c_uint64,
                                     ctypes.POINTER(ctypes.c_bool), _u64_p]
for _s, _r in FRI_HANDLE_SYMBOLS.items():
    getattr(lib, _s).restype = _r  # AttributeError if the symbol is missing
for _p in FRI_PREFIXES + FRI_WIDE_PREFIXES:
    getattr(lib, f"{_p}_icicle_initialize_fri_proof").argtypes = []
    getattr(lib, f"{_p}_icicle_create_with_arguments_fri_proof").argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                                             ctypes.c_uint64]
    getattr(lib, f"{_p}_icicle_delete_fri_proof").argtypes = [ctypes.c_void_p]
    for _s in ("fri_proof_get_nof_queries", "fri_proof_get_nof_rounds", "fri_proof_get_final_poly_size"):
        getattr(lib, f"{_p}_{_s}").argtypes = [ctypes.c_void_p, _size_p]
    getattr(lib, f"{_p}_fri_proof_get_round_proofs_for_query").argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    getattr(lib, f"{_p}_fri_proof_get_final_poly").argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    getattr(lib, f"{_p}_fri_proof_get_pow_nonce").argtypes = [ctypes.c_void_p, _u64_p]
    getattr(lib, f"{_p}_fri_merkle_tree_prove").argtypes = [ctypes.POINTER(FriConfig), ctypes.POINTER(FFIFriTranscriptConfig), ctypes.c_void_p, ctypes.c_size_t,
                                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    getattr(lib, f"{_p}_fri_merkle_tree_verify").argtypes = [ctypes.POINTER(FriConfig), ctypes.POINTER(FFIFriTranscriptConfig), ctypes.c_void_p, ctypes.c_void_p,
                                                             ctypes.c_void_p, ctypes.POINTER(ctypes.c_bool)]
    getattr(lib, f"{_p}_hip_fri_fold").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_bool, ctypes.c_void_p]
for _s, _r in SUMCHECK_HANDLE_SYMBOLS.items():
    getattr(lib, _s).restype = _r  # AttributeError if the symbol is missing
_void_pp = ctypes.POINTER(ctypes.c_void_p)
lib.delete_program.argtypes = [ctypes.c_void_p]
lib.icicle_hip_sumcheck_time_rounds.argtypes = [ctypes.c_bool]
lib.icicle_hip_sumcheck_round_times.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
lib.icicle_hip_sumcheck_launch_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
for _p in SUMCHECK_FIELDS:
    _prove_args = [ctypes.c_void_p, _void_pp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(FFISumcheckTranscriptConfig),
                   ctypes.POINTER(SumcheckConfig)]
    getattr(lib, f"{_p}_sumcheck_create").argtypes = []
    getattr(lib, f"{_p}_sumcheck_delete").argtypes = [ctypes.c_void_p]
    getattr(lib, f"{_p}_sumcheck_get_proof").argtypes = _prove_args
    getattr(lib, f"{_p}_hip_sumcheck_prove").argtypes = _prove_args + [ctypes.c_void_p]
    getattr(lib, f"{_p}_sumcheck_verify").argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(FFISumcheckTranscriptConfig),
                                                      ctypes.POINTER(ctypes.c_bool)]
    getattr(lib, f"{_p}_sumcheck_proof_create").argtypes = [_void_pp, ctypes.c_uint64, ctypes.c_uint64]
    getattr(lib, f"{_p}_sumcheck_proof_get_poly_sizes").argtypes = [ctypes.c_void_p, _u64_p, _u64_p]
    getattr(lib, f"{_p}_sumcheck_proof_get_round_poly_at").argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    getattr(lib, f"{_p}_sumcheck_proof_delete").argtypes = [ctypes.c_void_p]
    getattr(lib, f"{_p}_sumcheck_get_challenge_vector").argtypes = [ctypes.c_void_p, ctypes.c_void_p, _size_p]
    getattr(lib, f"{_p}_sumcheck_get_challenge_size").argtypes = [ctypes.c_void_p, _size_p]
    getattr(lib, f"{_p}_create_predefined_returning_value_program").argtypes = [ctypes.c_int]
    getattr(lib, f"{_p}_generate_returning_value_program").argtypes = [_void_pp, ctypes.c_int, _void_pp]
    getattr(lib, f"{_p}_create_input_symbol").argtypes = [ctypes.c_int]
    getattr(lib, f"{_p}_create_scalar_symbol").argtypes = [ctypes.c_void_p]
    getattr(lib, f"{_p}_copy_symbol").argtypes = [ctypes.c_void_p]
    for _s in ("add_symbols", "sub_symbols", "multiply_symbols"):
        getattr(lib, f"{_p}_{_s}").argtypes = [ctypes.c_void_p, ctypes.c_void_p, _void_pp]
    getattr(lib, f"{_p}_inverse_symbol").argtypes = [ctypes.c_void_p, _void_pp]
    getattr(lib, f"{_p}_create_predefined_program").restype = PROGRAM_HANDLE_SYMBOLS[f"{_p}_create_predefined_program"]
    getattr(lib, f"{_p}_create_predefined_program").argtypes = [ctypes.c_int]
    getattr(lib, f"{_p}_generate_program").argtypes = [_void_pp, ctypes.c_int, _void_pp]
    getattr(lib, f"{_p}_execute_program").argtypes = [_void_pp, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(VecOpsConfig)]


def multi_stats(reset=False):
    """dict of the multi-device / pipelined-path counters (icicle_hip_multi_stats)"""
    out = (ctypes.c_uint64 * 8)()
    check(lib.icicle_hip_multi_stats2(out, 8, reset), "multi_stats")
    return dict(zip(("staged_base_bytes", "staged_scalar_bytes", "exchanged_bucket_bytes", "resident_base_hits", "threaded_calls", "exchange_messages", "peer_staged_copies",
                     "plan_fallbacks"),
                    [int(v) for v in out]))
