"""Python model of execute_program as the reference's CPU backend computes it (include/icicle/program/program.h, backend/cpu/include/
cpu_program_executor.h, backend/cpu/src/field/cpu_vec_ops.cpp:635-678): the instruction list in the reference's order, run over
Python ints, and the lowering the kernel runs (icicle_amd/csrc/program_lower.h) stated over the same list. tests/golden/
execute_program_vectors.json holds the reference's own results."""
import json
import os

from tests.sumcheck_model import FIELDS, AB_MINUS_C, EQ_X_AB_MINUS_C  # noqa: F401

COPY, ADD, MUL, SUB, INV = 0, 1, 2, 3, 4  # ProgramOpcode
OPS = {"add": ADD, "mul": MUL, "sub": SUB, "inv": INV}
CAPS = {1: 64, 8: 24}  # values alive at once, by words of an element (program_lower.h)
MONT_BITS = {1: 32, 8: 261}


class VecProgram:
    """`nodes`: node j is ["in", i], ["const", value], [op, a, b] with op in add, sub, mul, or ["inv", a]; a, b are indices of earlier
    nodes. `params`: for every parameter the node whose value it has afterwards (["in", i] for a parameter i the program leaves
    alone). Or one of the two predefined programs."""

    def __init__(self, nof_parameters, nodes=None, params=None, predefined=None):
        self.nof_parameters, self.nodes, self.params, self.predefined = nof_parameters, nodes, params, predefined
        assert predefined is not None or len(params) == nof_parameters
        self._compiled = None  # the program is not changed after it is made

    @classmethod
    def from_description(cls, d):
        if "predefined" in d:
            return cls({AB_MINUS_C: 4, EQ_X_AB_MINUS_C: 5}[d["predefined"]], predefined=d["predefined"])
        return cls(d["nof_parameters"], [[n[0]] + [int(v, 16) if n[0] == "const" else v for v in n[1:]] for n in d["nodes"]], d["params"])

    def description(self):
        if self.predefined is not None:
            return {"predefined": self.predefined}
        return {"nof_parameters": self.nof_parameters, "params": self.params,
                "nodes": [[n[0]] + [f"{v:x}" if n[0] == "const" else v for v in n[1:]] for n in self.nodes]}

    def compile(self):
        """(instructions [op, a, b, dst] over variables, constants, number of intermediates): constants are numbered first, over all
        parameters' graphs in post-order; then parameter by parameter, each subtree in post-order, operand 1 before operand 2; the
        node of parameter i is computed into variable i, and copied there when it already lives elsewhere"""
        assert self.predefined is None
        if self._compiled is None:
            self._compiled = self._compile()
        ins, consts, inter = self._compiled
        return [list(i) for i in ins], list(consts), inter

    def _compile(self):
        np_, nodes = self.nof_parameters, self.nodes
        var, consts, seen = {}, [], set()

        def constants(j):
            if j in seen:
                return
            seen.add(j)
            n = nodes[j]
            if n[0] == "in":
                var[j] = n[1]
            elif n[0] == "const":
                var[j] = np_ + len(consts)
                consts.append(n[1])
            else:
                for a in n[1:]:
                    constants(a)

        for j in self.params:
            constants(j)
        ins, seen, inter = [], set(), [0]

        def emit(j):
            n = nodes[j]
            if n[0] in ("in", "const") or j in seen:
                return
            seen.add(j)
            for a in n[1:]:
                emit(a)
            if j not in var:
                var[j] = np_ + len(consts) + inter[0]
                inter[0] += 1
            ins.append([OPS[n[0]], var[n[1]], var[n[2]] if len(n) > 2 else 0, var[j]])

        for i, j in enumerate(self.params):
            if j not in var:
                var[j] = i
                emit(j)
            elif var[j] != i:
                ins.append([COPY, var[j], 0, i])
        return ins, consts, inter[0]

    def nof_vars(self):
        if self.predefined is not None:
            return self.nof_parameters
        _, consts, inter = self.compile()
        return self.nof_parameters + len(consts) + inter

    def evaluate(self, p, x):
        """the parameters' values of one element after the program ran over `x`"""
        x = list(x)
        if self.predefined == AB_MINUS_C:
            return x[:3] + [(x[0] * x[1] - x[2]) % p]
        if self.predefined == EQ_X_AB_MINUS_C:
            return x[:4] + [x[3] * (x[0] * x[1] - x[2]) % p]
        ins, consts, inter = self.compile()
        v = x + [c % p for c in consts] + [0] * inter
        for op, a, b, d in ins:
            v[d] = apply(p, op, v[a], v[b])
        return v[:self.nof_parameters]

    def written(self):
        if self.predefined is not None:
            return [self.nof_parameters - 1]
        return sorted({d for _, _, _, d in self.compile()[0] if d < self.nof_parameters})


def apply(p, op, a, b):
    if op == COPY:
        return a
    if op == INV:
        return pow(a, p - 2, p)  # 0 gives 0, as the reference's inverse does (the fixture's zero case)
    return (a + b if op == ADD else a - b if op == SUB else a * b) % p


def execute(field, program, data):
    """data: one list of ints per parameter -> the lists afterwards (a copy)"""
    p = FIELDS[field][0]
    if program.predefined is not None:
        rows = [program.evaluate(p, [d[i] for d in data]) for i in range(len(data[0]))]
    else:
        ins, consts, inter = program.compile()
        tail, rows = [c % p for c in consts] + [0] * inter, []
        for i in range(len(data[0])):
            v = [d[i] for d in data] + tail
            for op, a, b, dst in ins:
                v[dst] = apply(p, op, v[a], v[b])
            rows.append(v[:program.nof_parameters])
    return [[r[j] for r in rows] for j in range(len(data))]


# ---- the lowering (program_lower.h), over the same instruction list -----------------------------------------------------------------
LOAD, STORE = 8, 9


def lower(program, cap):
    """-> None when more than `cap` values are alive at once, else (code [op, a, b, dst] over slots, slots used, use per parameter:
    1 = read, 2 = written). Constant k lives in slot k; a parameter is loaded before the first instruction that reads its value from
    memory; a value takes the lowest free slot and gives it back after its last use; the written parameters are stored at the end."""
    ins, consts, inter = program.compile()
    np_, nc = program.nof_parameters, len(consts)
    nv = np_ + nc + inter
    is_const = lambda v: np_ <= v < np_ + nc
    ops, defined, use = [], [np_ <= v < np_ + nc for v in range(nv)], [0] * np_
    for op, a, b, d in ins:
        srcs = [a] if op in (COPY, INV) else [a, b]
        for v in srcs:
            if not defined[v]:
                assert v < np_
                ops.append((LOAD, v, -1, v))
                use[v] |= 1
                defined[v] = True
        ops.append((op, srcs[0], srcs[1] if len(srcs) > 1 else -1, d))
        defined[d] = True
        if d < np_:
            use[d] |= 2
    ops += [(STORE, j, j, -1) for j in range(np_) if use[j] & 2]
    after, live = [None] * len(ops), set()
    for k in range(len(ops) - 1, -1, -1):
        op, a, b, d = ops[k]
        after[k] = set(live)
        live.discard(d)
        if op != LOAD:
            live |= {v for v in ((a,) if op == STORE else (a, b)) if v >= 0 and not is_const(v)}
    if nc > cap:
        return None
    slot, used, peak, code = {np_ + k: k for k in range(nc)}, set(range(nc)), nc, []
    for k, (op, a, b, d) in enumerate(ops):
        sa = sb = sd = 0
        if op == LOAD:
            sa = a
        else:
            sa = slot[a]
            sb = b if op == STORE else (slot[b] if b >= 0 else 0)
            for v in ((a,) if op == STORE else (a, b)):
                if v >= 0 and not is_const(v) and v != d and v not in after[k] and v in slot:
                    used.discard(slot.pop(v))
        if d >= 0:
            if d not in slot:
                s = min(set(range(len(used) + 1)) - used)
                if s >= cap:
                    return None
                slot[d] = s
                used.add(s)
                peak = max(peak, s + 1)
            sd = slot[d]
            if d not in after[k]:
                used.discard(slot.pop(d))
        code.append([op, sa, sb, sd])
    return code, peak, use


def run_lowered(p, code, constants, x, nof_slots):
    """the lowered list over Python ints: x = the parameters' values in memory -> the values in memory afterwards"""
    mem, file = list(x), [c % p for c in constants] + [None] * (nof_slots - len(constants))
    for op, a, b, d in code:
        if op == LOAD:
            file[d] = mem[a]
        elif op == STORE:
            mem[b] = file[a]
        else:
            file[d] = apply(p, op, file[a], file[b])
    return mem


# ---- the fixtures (tests/golden/execute_program_vectors.json) -----------------------------------------------------------------------
def load_fixtures():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "execute_program_vectors.json")) as f:
        return json.load(f)["cases"]


def unhex(rows):
    return [[int(v, 16) for v in row] for row in rows]
