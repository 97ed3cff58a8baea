"""slice, highest_non_zero_idx, poly_eval and poly_division over Python integers, with the batch semantics the device implements
(include/icicle_hip.h): every size is per batch entry, entry k holds its element j at k * size + j, or at j * batch + k with columns.
Vectors are flat lists of integers below p. Errors are ValueError, where the library returns ICICLE_INVALID_ARGUMENT.

The reference (backend/cpu/src/field/cpu_vec_ops.cpp:566-780) agrees with this model wherever it is well defined; where it is not
(tests/test_poly_model_cpu.py pins that on the CPU) the model is the mathematically correct reading."""


def entry(vec, k, size, batch, columns):
    return [vec[j * batch + k] for j in range(size)] if columns else list(vec[k * size:(k + 1) * size])


def pack(entries, columns):
    """entries of one length -> the flat batch vector"""
    if not columns:
        return [v for e in entries for v in e]
    return [e[j] for j in range(len(entries[0])) for e in entries] if entries and entries[0] else []


def slice_(vec, offset, stride, size_in, size_out, batch=1, columns=False):
    if size_out == 0:
        return []
    if offset + (size_out - 1) * stride >= size_in:
        raise ValueError("slice out of bound")
    return pack([[e[offset + i * stride] for i in range(size_out)] for e in (entry(vec, k, size_in, batch, columns) for k in range(batch))], columns)


def degree(coeffs):
    for j in range(len(coeffs) - 1, -1, -1):
        if coeffs[j]:
            return j
    return -1


def highest_non_zero_idx(vec, size, batch=1, columns=False):
    if size == 0:
        raise ValueError("size == 0")
    return [degree(entry(vec, k, size, batch, columns)) for k in range(batch)]


def horner(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def poly_eval(p, coeffs, coeffs_size, domain, batch=1, columns=False):
    if coeffs_size == 0 or len(domain) == 0:
        raise ValueError("empty")
    return pack([[horner(entry(coeffs, k, coeffs_size, batch, columns), x, p) for x in domain] for k in range(batch)], columns)


def divmod_poly(p, num, den):
    """(q, r) as coefficient lists without trailing zeros beyond their degree (q of deg_n - deg_b + 1 entries, r of deg_b); den != 0"""
    dn, db = degree(num), degree(den)
    if db < 0:
        raise ValueError("zero denominator")
    r = list(num[:dn + 1])
    if dn < db:
        return [], r
    inv = pow(den[db], p - 2, p)
    q = [0] * (dn - db + 1)
    for m in range(dn - db, -1, -1):
        c = r[m + db] * inv % p
        q[m] = c
        if c:
            for j in range(db + 1):
                r[m + j] = (r[m + j] - c * den[j]) % p
    return q, r[:db]


def poly_division(p, num, num_size, den, den_size, q_size, r_size, batch=1, columns=False):
    """-> (q, r) flat, q_size / r_size elements per entry, zero above the degrees"""
    if num_size == 0 or den_size <= 0:
        raise ValueError("empty")
    ents = [(entry(num, k, num_size, batch, columns), entry(den, k, den_size, batch, columns)) for k in range(batch)]
    for n, d in ents:  # every entry is checked before anything is written
        dn, db = degree(n), degree(d)
        if db < 0 or r_size < dn + 1 or (dn - db + 1 > 0 and q_size < dn - db + 1):
            raise ValueError("degrees")
    qs, rs = [], []
    for n, d in ents:
        q, r = divmod_poly(p, n, d)
        qs.append(q + [0] * (q_size - len(q)))
        rs.append(r + [0] * (r_size - len(r)))
    return pack(qs, columns), pack(rs, columns)


def poly_mul(p, a, b):
    out = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % p
    return out
