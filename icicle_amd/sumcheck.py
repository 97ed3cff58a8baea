"""Sumcheck on the device over babybear, koalabear (one word per element) and the bn254, bls12_381 scalar fields (eight words):
mirror of wrappers/rust/icicle-core/src/{sumcheck,program,symbol} (Symbol, ReturningValueProgram, SumcheckConfig,
SumcheckTranscriptConfig, Sumcheck, SumcheckProof) over <field>_sumcheck_* / <field>_*_symbol(s) / <field>_*_program
(include/icicle_hip.h). Elements are canonical uint32 words: arrays of shape [n] (one word) or [n, 8]; a single element may also be
given as a Python int."""
import ctypes

import numpy as np

from ._lib import lib, check, SumcheckConfig, FFISumcheckTranscriptConfig, SUMCHECK_FIELDS
from .hash import _ptr

__all__ = ["Symbol", "ReturningValueProgram", "SumcheckConfig", "SumcheckTranscriptConfig", "Sumcheck", "SumcheckProof", "AB_MINUS_C", "EQ_X_AB_MINUS_C"]

AB_MINUS_C, EQ_X_AB_MINUS_C = 0, 1  # PreDefinedPrograms (include/icicle/program/program.h)


def _words(field):
    assert field in SUMCHECK_FIELDS, field
    return SUMCHECK_FIELDS[field]


def _fn(field, name):
    _words(field)
    return getattr(lib, f"{field}_{name}")


def _element(field, value):
    """one element as a ctypes array of words, from an int or a sequence of words"""
    w = _words(field)
    if isinstance(value, (int, np.integer)):
        v = int(value)
        assert 0 <= v < 1 << (32 * w), "element does not fit"
        words = [(v >> (32 * i)) & 0xFFFFFFFF for i in range(w)]
    else:
        words = [int(x) for x in np.asarray(value).reshape(-1)]
        assert len(words) <= w, "more words than an element has"
        words += [0] * (w - len(words))
    return (ctypes.c_uint32 * w)(*words)


class Symbol:
    """A node of the combine function's data-flow graph. The handle belongs to the library and lives until the next program is
    generated, which frees every symbol made so far."""

    def __init__(self, field, handle):
        if not handle:
            raise ValueError("symbol creation failed")
        self.field, self.handle = field, handle

    @classmethod
    def input(cls, field, index):
        return cls(field, _fn(field, "create_input_symbol")(index))

    @classmethod
    def constant(cls, field, value):
        return cls(field, _fn(field, "create_scalar_symbol")(_element(field, value)))

    def copy(self):
        return Symbol(self.field, _fn(self.field, "copy_symbol")(self.handle))

    def _binary(self, name, other, swap=False):
        if not isinstance(other, Symbol):
            other = Symbol.constant(self.field, other)
        a, b = (other, self) if swap else (self, other)
        out = ctypes.c_void_p()
        check(_fn(self.field, name)(a.handle, b.handle, ctypes.byref(out)), name)
        return Symbol(self.field, out.value)

    def __add__(self, other):
        return self._binary("add_symbols", other)

    def __radd__(self, other):
        return self._binary("add_symbols", other, swap=True)

    def __sub__(self, other):
        return self._binary("sub_symbols", other)

    def __rsub__(self, other):
        return self._binary("sub_symbols", other, swap=True)

    def __mul__(self, other):
        return self._binary("multiply_symbols", other)

    def __rmul__(self, other):
        return self._binary("multiply_symbols", other, swap=True)

    def inverse(self):
        out = ctypes.c_void_p()
        check(_fn(self.field, "inverse_symbol")(self.handle, ctypes.byref(out)), "inverse_symbol")
        return Symbol(self.field, out.value)


class ReturningValueProgram:
    """A combine function: owns a program handle."""

    def __init__(self, field, handle, nof_inputs):
        if not handle:
            raise ValueError("program creation failed")
        self.field, self.handle, self.nof_inputs = field, handle, nof_inputs

    @classmethod
    def predefined(cls, field, program_id):
        return cls(field, _fn(field, "create_predefined_returning_value_program")(program_id), {AB_MINUS_C: 3, EQ_X_AB_MINUS_C: 4}.get(program_id, 0))

    @classmethod
    def from_function(cls, field, fn, nof_inputs):
        """fn(inputs: list of Symbol) -> Symbol (an int return value becomes a constant)"""
        inputs = [Symbol.input(field, i) for i in range(nof_inputs)]
        result = fn(list(inputs))
        if not isinstance(result, Symbol):
            result = Symbol.constant(field, result)
        params = (ctypes.c_void_p * (nof_inputs + 1))(*[s.handle for s in inputs], result.handle)
        out = ctypes.c_void_p()
        check(_fn(field, "generate_returning_value_program")(params, nof_inputs + 1, ctypes.byref(out)), "generate_returning_value_program")
        return cls(field, out.value, nof_inputs)

    def close(self):
        if self.handle is not None:
            check(lib.delete_program(self.handle), "delete_program")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SumcheckTranscriptConfig:
    """Hasher, labels and seed of the Fiat-Shamir transcript. `seed_rng`: one element, an int or a sequence of words."""

    def __init__(self, hasher, domain_separator_label, round_poly_label, round_challenge_label, seed_rng, little_endian=True):
        as_bytes = lambda s: s.encode() if isinstance(s, str) else bytes(s)
        self.hasher = hasher
        self.domain_separator_label = as_bytes(domain_separator_label)
        self.round_poly_label = as_bytes(round_poly_label)
        self.round_challenge_label = as_bytes(round_challenge_label)
        self.seed_rng, self.little_endian = seed_rng, little_endian

    def _ffi(self, field):
        """(struct, objects that must outlive the call)"""
        labels = (self.domain_separator_label, self.round_poly_label, self.round_challenge_label)
        keep = [ctypes.create_string_buffer(b, max(len(b), 1)) for b in labels]
        seed = _element(field, self.seed_rng)
        args = [self.hasher.handle if self.hasher is not None else None]
        for buf, b in zip(keep, labels):
            args += [ctypes.cast(buf, ctypes.c_void_p), len(b)]
        return FFISumcheckTranscriptConfig(*args, self.little_endian, ctypes.cast(seed, ctypes.c_void_p)), keep + [seed]


class SumcheckProof:
    """Owns a proof handle: the round polynomials, d + 1 evaluations each."""

    def __init__(self, field, handle=None):
        self.field = field
        self.handle = handle or _fn(field, "sumcheck_proof_create")(None, 0, 0)
        if not self.handle:
            raise MemoryError("sumcheck proof creation failed")

    @classmethod
    def create(cls, field, polys):
        """polys: array [rounds, d + 1] (one word) or [rounds, d + 1, 8], or a list of such rows"""
        w = _words(field)
        rows = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1) for p in polys]
        size = rows[0].size // w if rows else 0
        assert all(r.size == size * w for r in rows), "round polynomials of different lengths"
        table = (ctypes.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows])
        h = _fn(field, "sumcheck_proof_create")(table, len(rows), size)
        if not h:
            raise MemoryError("sumcheck proof creation failed")
        return cls(field, h)

    def sizes(self):
        """(evaluations per round polynomial, number of round polynomials)"""
        size, count = ctypes.c_uint64(), ctypes.c_uint64()
        check(_fn(self.field, "sumcheck_proof_get_poly_sizes")(self.handle, ctypes.byref(size), ctypes.byref(count)), "sumcheck_proof_get_poly_sizes")
        return int(size.value), int(count.value)

    def round_polys(self) -> np.ndarray:
        """uint32 [rounds, d + 1] or [rounds, d + 1, 8], a copy"""
        w = _words(self.field)
        size, count = self.sizes()
        out = np.zeros((count, size, w), dtype=np.uint32)
        for r in range(count):
            p = _fn(self.field, "sumcheck_proof_get_round_poly_at")(self.handle, r)
            out[r] = np.frombuffer(ctypes.string_at(p, 4 * size * w), dtype=np.uint32).reshape(size, w)
        return out.reshape(count, size) if w == 1 else out

    def close(self):
        if self.handle is not None:
            check(_fn(self.field, "sumcheck_proof_delete")(self.handle), "sumcheck_proof_delete")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sumcheck:
    """Prover and verifier of one field; remembers the challenge vector of its last proof."""

    def __init__(self, field):
        self.field = field
        self.handle = _fn(field, "sumcheck_create")()
        if not self.handle:
            raise MemoryError("sumcheck creation failed")

    def prove(self, polys, claimed_sum, program, tcfg, cfg=None) -> SumcheckProof:
        """polys: the MLE polynomials, all NumPy uint32 arrays on the host or all DeviceVec, 2^L elements each. Returns with
        cfg.stream drained."""
        w = _words(self.field)
        cfg = SumcheckConfig.from_buffer_copy(cfg) if cfg is not None else SumcheckConfig.default()  # the caller's config stays as it is
        ptrs = [_ptr(p) for p in polys]
        assert ptrs and len({d for _, d in ptrs}) == 1, "polynomials must be all on the host or all on the device"
        assert len({p.nbytes for p in polys}) == 1, "polynomials of different sizes"
        cfg.are_inputs_on_device = ptrs[0][1]
        table = (ctypes.c_void_p * len(ptrs))(*[a for a, _ in ptrs])
        ffi, keep = tcfg._ffi(self.field)
        proof = SumcheckProof(self.field)
        check(_fn(self.field, "hip_sumcheck_prove")(self.handle, table, polys[0].nbytes // (4 * w), len(ptrs), _element(self.field, claimed_sum), program.handle,
                                                    ctypes.byref(ffi), ctypes.byref(cfg), proof.handle), "hip_sumcheck_prove")
        del keep
        return proof

    def verify(self, proof, claimed_sum, tcfg) -> bool:
        ffi, keep = tcfg._ffi(self.field)
        ok = ctypes.c_bool(False)
        check(_fn(self.field, "sumcheck_verify")(self.handle, proof.handle, _element(self.field, claimed_sum), ctypes.byref(ffi), ctypes.byref(ok)), "sumcheck_verify")
        del keep
        return bool(ok.value)

    def challenge_vector(self) -> np.ndarray:
        """alpha_0 = 0, alpha_1, ..: uint32 [rounds] or [rounds, 8]"""
        w = _words(self.field)
        n = ctypes.c_size_t()
        check(_fn(self.field, "sumcheck_get_challenge_size")(self.handle, ctypes.byref(n)), "sumcheck_get_challenge_size")
        out = np.zeros((n.value, w), dtype=np.uint32)
        if n.value:
            check(_fn(self.field, "sumcheck_get_challenge_vector")(self.handle, out.ctypes.data, ctypes.byref(n)), "sumcheck_get_challenge_vector")
        return out.reshape(-1) if w == 1 else out

    def close(self):
        if self.handle is not None:
            check(_fn(self.field, "sumcheck_delete")(self.handle), "sumcheck_delete")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

