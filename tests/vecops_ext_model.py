"""The two extension fields of the extension vector operations in Python integers, written from the definitions.

babybear, koalabear: F[x] / (x^4 - W), W = 11 and 3 (fields/stark_fields/babybear.h, koalabear.h: nonresidue), an element is a tuple of
four coefficients, constant term first. goldilocks: c0 + c1 u, u^2 = 7, a tuple of two. Memory layout: every coefficient canonical
and little-endian, 4 or 8 bytes, 16 bytes per element.

inv() goes through the norm (the tower x^2 = y, y^2 = W for the quartic field); inv_fermat() is a second way, a^(q - 2) by square and
multiply in the model itself, q = p^degree. The inverse of zero is zero either way."""
import numpy as np

from oracle import pyref

FIELDS = ("babybear", "koalabear", "goldilocks")
DEGREE = {"babybear": 4, "koalabear": 4, "goldilocks": 2}
BASE_WORDS = {"babybear": 1, "koalabear": 1, "goldilocks": 2}
# pyref carries the moduli; it has no table of the extensions' non-residues, so they are stated here
NONRES = getattr(pyref, "EXT_NONRES", {"babybear": 11, "koalabear": 3, "goldilocks": 7})


def modulus(f):
    return pyref.NTT_FIELDS[f].p


def zero(f):
    return (0,) * DEGREE[f]


def one(f):
    return (1,) + (0,) * (DEGREE[f] - 1)


def embed(f, b):
    return (b % modulus(f),) + (0,) * (DEGREE[f] - 1)


def add(f, a, b):
    p = modulus(f)
    return tuple((x + y) % p for x, y in zip(a, b))


def sub(f, a, b):
    p = modulus(f)
    return tuple((x - y) % p for x, y in zip(a, b))


def mul(f, a, b):
    """the product of two polynomials, reduced by x^d = W"""
    p, d, w = modulus(f), DEGREE[f], NONRES[f]
    r = [0] * d
    for i in range(d):
        for j in range(d):
            if i + j < d:
                r[i + j] += a[i] * b[j]
            else:
                r[i + j - d] += w * a[i] * b[j]
    return tuple(v % p for v in r)


def mul_base(f, a, b):
    p = modulus(f)
    return tuple(x * b % p for x in a)


def _quad_norm_inv(p, w, a0, a1):
    """(a0 + a1 t)^-1 with t^2 = w over F_p: (a0 - a1 t) / (a0^2 - w a1^2); zero for zero"""
    n = (a0 * a0 - w * a1 * a1) % p
    ni = pow(n, p - 2, p)
    return a0 * ni % p, (-a1 * ni) % p


def inv(f, a):
    """through the norm; inv(0) = 0"""
    p, w = modulus(f), NONRES[f]
    if DEGREE[f] == 2:
        return _quad_norm_inv(p, w, a[0], a[1])
    # a = A + x B over K = F[y] / (y^2 - W), A = a0 + a2 y, B = a1 + a3 y, x^2 = y: a^-1 = (A - x B) / (A^2 - y B^2)
    def kmul(u, v):
        return ((u[0] * v[0] + w * u[1] * v[1]) % p, (u[0] * v[1] + u[1] * v[0]) % p)

    A, B = (a[0], a[2]), (a[1], a[3])
    BB = kmul(B, B)
    AA = kmul(A, A)
    n = ((AA[0] - w * BB[1]) % p, (AA[1] - BB[0]) % p)  # A^2 - y B^2, in K
    ni = _quad_norm_inv(p, w, n[0], n[1])
    ra, rb = kmul(A, ni), kmul(B, ni)
    return (ra[0], (-rb[0]) % p, ra[1], (-rb[1]) % p)


def power(f, a, e):
    r, base = one(f), a
    while e:
        if e & 1:
            r = mul(f, r, base)
        base = mul(f, base, base)
        e >>= 1
    return r


def inv_fermat(f, a):
    """a^(q - 2), q = p^degree: the group of units has q - 1 elements, and zero stays zero"""
    return power(f, a, modulus(f) ** DEGREE[f] - 2)


def div(f, a, b):
    return mul(f, a, inv(f, b))


def vsum(f, elems):
    r = zero(f)
    for e in elems:
        r = add(f, r, e)
    return r


def vproduct(f, elems):
    r = one(f)
    for e in elems:
        r = mul(f, r, e)
    return r


def reduce_np(f, op, a, size, batch, columns):
    """vector_sum / vector_product of `batch` entries of `size` elements each, given as [size * batch, 4] words of a field with a one-word
    base field: vsum / vproduct above in uint64 arithmetic (p < 2^31, every product reduced before it is added), all entries at once.
    Returns [batch, 4] words."""
    assert BASE_WORDS[f] == 1 and op in ("vector_sum", "vector_product")
    p, w, d = np.uint64(modulus(f)), np.uint64(NONRES[f]), DEGREE[f]
    x = np.ascontiguousarray(a, np.uint32).reshape((size, batch, d) if columns else (batch, size, d)).astype(np.uint64)
    rows = x.transpose(1, 0, 2) if columns else x  # [batch, size, d]
    if op == "vector_sum":
        return (rows.sum(axis=1) % p).astype(np.uint32)  # size < 2^33
    acc = rows[:, 0, :].copy()
    for j in range(1, size):
        r = np.zeros_like(acc)
        for i in range(d):
            for k in range(d):
                t = acc[:, i] * rows[:, j, k] % p
                if i + k < d:
                    r[:, i + k] += t
                else:
                    r[:, i + k - d] += w * t % p
        acc = r % p
    return acc.astype(np.uint32)


# ---- memory layout ------------------------------------------------------------------------------------------------------------------
def to_words(f, elems):
    """[n, 4] uint32"""
    cb = 4 * BASE_WORDS[f]
    return np.frombuffer(b"".join(int(c).to_bytes(cb, "little") for e in elems for c in e), np.uint32).reshape(-1, 4).copy()


def from_words(f, arr):
    cb, d = 4 * BASE_WORDS[f], DEGREE[f]
    raw = np.ascontiguousarray(arr, np.uint32).tobytes()
    vals = [int.from_bytes(raw[i:i + cb], "little") for i in range(0, len(raw), cb)]
    return [tuple(vals[i:i + d]) for i in range(0, len(vals), d)]


def base_to_words(f, vals):
    w = BASE_WORDS[f]
    return np.frombuffer(b"".join(int(v).to_bytes(4 * w, "little") for v in vals), np.uint32).reshape(-1, w).copy()


def to_hex(f, elems):
    return to_words(f, elems).tobytes().hex()


def from_hex(f, s):
    return from_words(f, np.frombuffer(bytes.fromhex(s), np.uint32))


# ---- the twelve functions over whole vectors ---------------------------------------------------------------------------------------
OPS_2 = ("vector_add", "vector_sub", "vector_mul", "vector_div", "vector_mixed_mul", "scalar_add_vec", "scalar_sub_vec", "scalar_mul_vec")
OPS_1 = ("vector_inv", "vector_sum", "vector_product", "bit_reverse")


def entry_index(j, k, size, batch, columns):
    """where element j of batch entry k lies"""
    return j * batch + k if columns else k * size + j


def run(f, op, a, b=None, size=None, batch=1, columns=False):
    """op over lists of elements, as the C functions define it; for vector_mixed_mul b is a list of base-field integers, for scalar_*
    a holds one scalar per batch entry"""
    fn2 = {"vector_add": add, "vector_sub": sub, "vector_mul": mul, "vector_div": div}
    if op in fn2:
        return [fn2[op](f, x, y) for x, y in zip(a, b)]
    if op == "vector_mixed_mul":
        return [mul_base(f, x, y) for x, y in zip(a, b)]
    if op == "vector_inv":
        return [inv(f, x) for x in a]
    if op.startswith("scalar_"):
        g = {"scalar_add_vec": add, "scalar_sub_vec": sub, "scalar_mul_vec": mul}[op]
        out = list(b)
        for k in range(batch):
            for j in range(size):
                i = entry_index(j, k, size, batch, columns)
                out[i] = g(f, a[k], b[i])
        return out
    if op in ("vector_sum", "vector_product"):
        g = vsum if op == "vector_sum" else vproduct
        return [g(f, [a[entry_index(j, k, size, batch, columns)] for j in range(size)]) for k in range(batch)]
    if op == "bit_reverse":
        logn = size.bit_length() - 1
        out = list(a)
        for k in range(batch):
            for j in range(size):
                r = int(format(j, f"0{logn}b")[::-1], 2) if logn else 0
                out[entry_index(r, k, size, batch, columns)] = a[entry_index(j, k, size, batch, columns)]
        return out
    raise ValueError(op)
