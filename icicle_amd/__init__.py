"""icicle_amd: MI355X (gfx950) backend for ICICLE's MSM / NTT hot path.

The product is libicicle_hip.so (hand-written HIP, C ABI in include/icicle_hip.h); this package is
the thin host-side mirror of the reference's wrapper API (wrappers/rust/icicle-core/src/{msm,ntt},
icicle-runtime) used by the tests and bench.py. There is no CPU fallback anywhere in here.
"""
from ._lib import IcicleError, Device, MSMConfig, NTTConfigU32, NTTConfigU64, NTTConfigU256, NTTInitDomainConfig, VecOpsConfig, HashConfig, MerkleTreeConfig, PowConfig, FriConfig, SumcheckConfig, lib, LIB_PATH  # noqa: F401
from . import runtime, msm, ntt, vecops, hash, merkle, fri, sumcheck, program  # noqa: F401
from .pow import pow_solve, pow_verify  # noqa: F401
from .fri import FriTranscriptConfig, FriProof, fri_merkle_tree_prove, fri_merkle_tree_verify  # noqa: F401
from .sumcheck import Symbol, ReturningValueProgram, SumcheckTranscriptConfig, Sumcheck, SumcheckProof  # noqa: F401
from .program import Program  # noqa: F401
from .vecops import execute_program, vector_inv, vector_div, vector_sum, vector_product, vector_mixed_mul, highest_non_zero_idx, poly_eval, poly_division  # noqa: F401

__all__ = ["runtime", "msm", "ntt", "vecops", "hash", "merkle", "fri", "sumcheck", "program", "Symbol", "ReturningValueProgram", "Program", "execute_program", "vector_inv", "vector_div", "vector_sum", "vector_product", "SumcheckConfig", "SumcheckTranscriptConfig", "Sumcheck", "SumcheckProof", "pow_solve", "pow_verify", "FriConfig", "FriTranscriptConfig", "FriProof", "fri_merkle_tree_prove", "fri_merkle_tree_verify", "HashConfig", "MerkleTreeConfig", "PowConfig", "VecOpsConfig", "IcicleError", "Device", "MSMConfig", "NTTConfigU32", "NTTConfigU64", "NTTConfigU256", "NTTInitDomainConfig", "vector_mixed_mul", "highest_non_zero_idx", "poly_eval", "poly_division"]
