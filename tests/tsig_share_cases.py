"""The seeded corpus of the threshold DSA / ECDSA share-answer tests (CPU and GPU).  Not collected.

    scalars(q, w, windows, width)     the ai classes: (label, value) with value < 2^(8 width), most of them below q
    requests(q, width, m, w, windows, seed) -> [(label, [(k, a, b, c)] * m)]: every ai class and every sum class, once each
    shares_array(reqs, width)         -> uint8 [n_reqs, m, 4, width]
    s_cases(q, nbytes, seed)          phase 3: [(label, m, r, y, k, c)]
    dsa_groups() / curves()           the groups of the tests: dsa1024, dsa2048 (tests/dsa_verify_cases.py); the four curves

A share column of a request sums, mod q, to what its label says; the other three columns are random below q unless the label
covers them."""
import random

import numpy as np

import dsa_verify_cases as DK
import ec_ref as E

DSA_NAMES = ("dsa1024", "dsa2048")
N_RANDOM = 32


def dsa_groups():
    return {name: DK.group(name) for name in DSA_NAMES}


def curves():
    return {name: E.CURVES[name] for name in E.NAMES}


def windows_of(q, w):
    return (q.bit_length() + w - 1) // w


def scalars(q, w, windows, width, seed=1):
    """0, 1, 2, 15, 16, q - 1; one non-zero digit in each window position; all digits 15 (2^w - 1 at other widths); all but the top
    window zero; N_RANDOM random ones.  A value at or above q is left as it is where the row holds it (the fold reduces it)."""
    rng = random.Random(seed * 7919 + w)
    cap = 1 << (8 * width)
    out = [("zero", 0), ("one", 1), ("two", 2), ("fifteen", 15), ("sixteen", 16), ("q_minus_1", q - 1)]
    for i in range(windows):
        d = rng.randrange(1, 1 << w)
        v = d << (w * i)
        if v >= q:
            v = 1 << (w * i)
        if v < cap and v < q:
            out.append(("digit@%d" % i, v))
    out.append(("all_max", min(cap, 1 << (w * windows)) - 1))
    top = 1 << (w * (windows - 1))
    out.append(("top_only", top if top < q else 1 << (q.bit_length() - 1)))
    out += [("random%d" % i, rng.randrange(q)) for i in range(N_RANDOM)]
    return out


SUM_CLASSES = ("wrap", "sum_q", "sum_0", "sum_1", "above_q")


def _column(rng, q, m, target):
    """m values below q whose sum is target mod q"""
    col = [rng.randrange(q) for _ in range(m - 1)]
    return col + [(target - sum(col)) % q]


def requests(q, width, m, w, windows, seed=1):
    rng = random.Random(seed * 104729 + m * 31 + w)
    cap = 1 << (8 * width)
    out = []
    for label, v in scalars(q, w, windows, width, seed):
        cols = [_column(rng, q, m, rng.randrange(q)) for _ in range(4)]
        if v < q:
            cols[1] = _column(rng, q, m, v)
        else:                                       # one share holds it whole, the others add nothing
            cols[1] = [v] + [0] * (m - 1)
        out.append(("a:" + label, list(zip(*cols))))
    for label in SUM_CLASSES:
        if label == "wrap":                         # m shares of q - 1 in every column: m - 1 wraps
            cols = [[q - 1] * m for _ in range(4)]
        elif label == "sum_q":                      # the plain sum is exactly q
            cols = [([q - 1, 1] + [0] * (m - 2)) if m > 1 else [q if q < cap else 0] for _ in range(4)]
        elif label == "sum_0":
            cols = [[0] * m for _ in range(4)]
        elif label == "sum_1":
            cols = [[0] * (m - 1) + [1] for _ in range(4)]
        else:                                       # every share in [q, 2^(8 width))
            cols = [[rng.randrange(q, cap) if cap > q else q - 1 for _ in range(m)] for _ in range(4)]
        out.append(("s:" + label, list(zip(*cols))))
    return out


def shares_array(reqs, width):
    """reqs: [[(k, a, b, c)] * m] -> uint8 [n_reqs, m, 4, width]"""
    raw = b"".join(int(v).to_bytes(width, "big") for sh in reqs for tup in sh for v in tup)
    return np.frombuffer(raw, dtype=np.uint8).reshape(len(reqs), len(reqs[0]), 4, width).copy()


def s_cases(q, nbytes, seed=1):
    """Operands at 0, 1, q - 1 and above q; r y + m and (..) k + c each landing exactly on q; random ones."""
    rng = random.Random(seed * 15485863 + nbytes)
    cap = 1 << (8 * nbytes)
    above = lambda: rng.randrange(q, cap) if cap > q else q - 1      # noqa: E731
    edge = [0, 1, q - 1, above()]
    out = []
    for pos in range(5):
        for e in edge:
            ops = [rng.randrange(q) for _ in range(5)]
            ops[pos] = e
            out.append(("edge%d" % pos, *ops))
    for e in edge:
        out.append(("all_edge", e, e, e, e, e))
    for _ in range(4):
        r, y, k = rng.randrange(1, q), rng.randrange(1, q), rng.randrange(1, q)
        m = (q - r * y % q) % q or q                                         # (q itself fits its row: q < 2^(8 nbytes))
        c_any = rng.randrange(q)
        out.append(("inner_on_q", m, r, y, k, c_any))                  # r y + m = q exactly (m = q itself where r y = 0 mod q)
        m2 = rng.randrange(q)
        t = (r * y % q + m2) % q * k % q
        out.append(("outer_on_q", m2, r, y, k, (q - t) % q if t else q))
    out.append(("all_above", above(), above(), above(), above(), above()))
    out += [("random", *[rng.randrange(q) for _ in range(5)]) for _ in range(8)]
    return out
