"""Programs with any number of outputs, for vecops.execute_program: mirror of wrappers/rust/icicle-core/src/program (Program) over
<field>_create_predefined_program / <field>_generate_program (include/icicle_hip.h). The symbols are sumcheck.Symbol."""
import ctypes

from ._lib import lib, check
from .sumcheck import Symbol, AB_MINUS_C, EQ_X_AB_MINUS_C, _fn

__all__ = ["Program"]


class Program:
    """A function of nof_parameters vectors, any of which it may read, write or both: owns a program handle."""

    def __init__(self, field, handle, nof_parameters):
        if not handle:
            raise ValueError("program creation failed")
        self.field, self.handle, self.nof_parameters = field, handle, nof_parameters

    @classmethod
    def predefined(cls, field, program_id):
        """AB_MINUS_C: parameters A, B, C and the output; EQ_X_AB_MINUS_C: A, B, C, E and the output"""
        return cls(field, _fn(field, "create_predefined_program")(program_id), {AB_MINUS_C: 4, EQ_X_AB_MINUS_C: 5}.get(program_id, 0))

    @classmethod
    def from_function(cls, field, fn, nof_parameters):
        """fn(x: list of Symbol) assigns the outputs in place, x[3] = x[0] * x[1] - x[2] (an int becomes a constant); a parameter it
        leaves alone stays what it was"""
        params = [Symbol.input(field, i) for i in range(nof_parameters)]
        fn(params)
        assert len(params) == nof_parameters, "the function must keep the list's length"
        params = [s if isinstance(s, Symbol) else Symbol.constant(field, s) for s in params]
        table = (ctypes.c_void_p * nof_parameters)(*[s.handle for s in params])
        out = ctypes.c_void_p()
        check(_fn(field, "generate_program")(table, nof_parameters, ctypes.byref(out)), "generate_program")
        return cls(field, out.value, nof_parameters)

    def close(self):
        if self.handle is not None:
            check(lib.delete_program(self.handle), "delete_program")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
