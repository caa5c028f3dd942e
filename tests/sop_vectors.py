"""Shared test vectors and exact-integer checks for the SOP arithmetic cores (csrc/lcv_col28.hpp sop_mac28 /
sop_kara_mac / sop_kara_join / sop_redc28 / fp_mul_c28 / fp_sqr_c28, csrc/lcv_sop.hpp sop_reduce).  The
generators are deterministic (fixed seeds) and return plain Python integers; the check_* functions compare what
the C++ returned with Python integers and are shared by the CPU twins (g++ -DLCV_HOSTSIM:
test_sop_reduce_cpu.py, test_col28_cpu.py, test_sop_arith_cpu.py) and the device run (build/soptest:
test_sop_arith_gpu.py), so both assert the same thing.  pack_input / unpack_output speak soptest's file format
(tools/microbench/soptest.hip)."""
import functools
import os
import random
import struct
import sys

import helpers as H

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import gen_sop as GS  # noqa: E402

P = GS.P
R = 1 << 384
RINV = pow(R, -1, P)
PINV = pow(P, -1, R)
M28 = (1 << 28) - 1
NP28 = (-pow(P, -1, 1 << 28)) % (1 << 28)
PL28 = [(P >> (28 * j)) & M28 for j in range(14)]
KMAX = 15  # products per columns record (soptest.hip): the round header's K has four bits


# ---------------------------------------------------------------------------------------------- reduce
@functools.lru_cache(maxsize=None)
def reduce_cases():
    """(value, red, use_table), value < 2^red p: on and around every multiple k p (sampled k for red > 5: the
    smallest and the largest 24 and 100 random ones; tools/gen_sop.py allows red <= 10, the error analysis needs
    q < 2^15), around the skip threshold (fractional part of the quotient estimate within ~2^-29 of 1), and 300
    random values; with the q p table (red <= 3 only) and without."""
    cases = []
    for red in range(1, 11):
        rng = random.Random(100 + red)
        top = (1 << red) * P
        vals = [0, 1, P - 1, top - 1, top - P]
        ks = range(1, 1 << red)
        if red > 5:
            ks = sorted(set(list(range(1, 25)) + list(range((1 << red) - 24, 1 << red)) +
                            [rng.randrange(1, 1 << red) for _ in range(100)]))
        for k in ks:
            vals += [k * P - 1, k * P, k * P + 1, k * P + (1 << 320) - 1, k * P - (1 << 320),
                     k * P + rng.randrange(1 << 64), k * P - rng.randrange(1, 1 << 64)]
            for f in (27, 28, 29, 30, 31, 32, 36):
                vals += [(k + 1) * P - (P >> f), k * P + (P >> f), (k + 1) * P - (P >> f) - 1]
        vals += [rng.randrange(top) for _ in range(300)]
        for use_table in ((0, 1) if red <= 3 else (0,)):
            cases += [(v, red, use_table) for v in vals if 0 <= v < top]
    return cases


def check_reduce(case, words):
    """words: the 13 words sop_reduce left."""
    v, red, use_table = case
    got = sum(int(w) << (32 * i) for i, w in enumerate(words[:12]))
    assert got == v % P and int(words[12]) == 0, (red, use_table, hex(v))


# ---------------------------------------------------------------------------------------------- c28
def limb_patterns():
    """Montgomery-limb patterns below 2p: every 28-bit limb saturated, single limb / word boundaries, runs of
    ones up to a limb boundary, p less a limb unit (a borrow through the low limbs), alternating saturated and
    zero limbs."""
    pats = [(1 << 380) - 1]
    pats += [1 << (28 * k) for k in range(14)]
    pats += [(1 << (28 * k)) - 1 for k in range(1, 14)]
    pats += [1 << (32 * k) for k in range(12)]
    pats += [P - (1 << (28 * k)) for k in range(14)]
    pats += [sum(M28 << (28 * i) for i in range(0, 14, 2)),
             sum(M28 << (28 * i) for i in range(1, 14, 2)) & ((1 << 380) - 1)]
    out = []
    for v in pats:
        assert 0 <= v < 2 * P
        if v not in out:
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def c28_cases():
    """Operand pairs (a, b), both below 2p (the range the column engine claims to accept): edges, lazily reduced
    values in [p, 2p), reduced values and the limb patterns; every value meets two others and itself."""
    rng = random.Random(28)
    edge = [0, 1, 2, P - 1, P, P + 1, 2 * P - 2, 2 * P - 1, (1 << 381) - 1, (1 << 381), 2 * P - (1 << 200)]
    vals = edge + [rng.randrange(P, 2 * P) for _ in range(60)] + [rng.randrange(P) for _ in range(20)]
    pairs = []
    for i, a in enumerate(vals):
        pairs += [(a, vals[(7 * i + 3) % len(vals)]), (a, vals[(5 * i + 1) % len(vals)]), (a, a)]
    pats = limb_patterns()
    allv = vals + pats
    for i, a in enumerate(pats):
        pairs += [(a, pats[(7 * i + 3) % len(pats)]), (a, allv[(5 * i + 1) % len(allv)]), (a, a)]
    return pairs


def check_c28(case, mul, sqr):
    """mul / sqr: the 13 words of fp_mul_c28(a, b) / fp_sqr_c28(a)."""
    a, b = case
    got = sum(int(w) << (32 * i) for i, w in enumerate(mul))
    assert got < 2 * P, (hex(a), hex(b))
    assert got % P == a * b * RINV % P, (hex(a), hex(b))
    got = sum(int(w) << (32 * i) for i, w in enumerate(sqr))
    assert got < 2 * P and got % P == a * a * RINV % P, hex(a)


# ---------------------------------------------------------------------------------------------- columns
def limbs28(v, n):
    return [(v >> (28 * i)) & M28 for i in range(n - 1)] + [v >> (28 * (n - 1))]


def exact_columns(prods, x15):
    """The 28 exact column sums: the plain convolution of the operands' 28-bit limbs."""
    nx = 15 if x15 else 14
    col = [0] * 28
    for X, Y in prods:
        x, y = limbs28(X, nx), limbs28(Y, 14)
        for i in range(nx):
            for j in range(14):
                col[i + j] += x[i] * y[j]
    return col


def exact_redc(prods):
    T = sum(x * y for x, y in prods)
    M = (-T * PINV) % R
    assert (T + M * P) % R == 0
    return (T + M * P) // R


def _assert_contract(prods, kara, x15):
    """The engine's contract, with exact integers: operands fit their limbs, no unsigned column (through the
    reduction's multiply-adds) reaches 2^64, no signed Karatsuba middle column reaches 2^63 (at any point of the
    accumulation), the reduced value fits 13 words."""
    assert 1 <= len(prods) <= KMAX and not (kara and x15)
    for X, Y in prods:
        assert 0 <= X < 1 << (416 if x15 else 392) and 0 <= Y < 1 << 384
    col = exact_columns(prods, x15)
    assert max(col) < 1 << 64
    if kara:
        p0, p2, pd = [0] * 13, [0] * 13, [0] * 13
        for X, Y in prods:
            x, y = limbs28(X, 14), limbs28(Y, 14)
            for i in range(7):
                for j in range(7):
                    p0[i + j] += x[i] * y[j]
                    p2[i + j] += x[i + 7] * y[j + 7]
                    pd[i + j] += (x[i] - x[i + 7]) * (y[j + 7] - y[j])
                    assert abs(pd[i + j]) < 1 << 63
        assert max(p0) < 1 << 64 and max(p2) < 1 << 64
    # the reduction: every column takes at most 14 quotient-digit products and a carry
    carry = 0
    for i in range(14):
        v = col[i] + carry
        q = (v * NP28) & (M28 if i < 13 else 0xFFFFF)
        assert v + q * PL28[0] < 1 << 64
        carry = (v + q * PL28[0]) >> 28 if i < 13 else 0
        if i == 13:
            col[13] = v + q * PL28[0]
        for j in range(1, 14):
            col[i + j] += q * PL28[j]
            assert col[i + j] < 1 << 64
    carry = 0
    for c in range(13, 28):
        assert col[c] + carry < 1 << 64
        carry = (col[c] + carry) >> 28
    assert exact_redc(prods) < 1 << 416


def op_shapes():
    """Every distinct op shape ((m, X terms, Y terms) per product, x15, kara) of the four generated programs."""
    shapes = []
    for p in GS.build():
        p.finalize()
        for ops in p.rounds:
            x15, kara = p.round_flags(ops)
            for o in ops:
                key = (tuple((m, len(x), len(y)) for x, y, m in o.prods), bool(x15), bool(kara))
                if key[0] and key not in shapes:
                    shapes.append(key)
    assert shapes
    return shapes


@functools.lru_cache(maxsize=None)
def column_cases():
    """(prods, kara, x15), prods = [(X, Y)] as the device forms them (X = m (t0 + t1), Y = t0 + t1).  For every
    op shape of the programs: every term p (the largest a term can be: the shadow of 0), every term p - 1, terms
    alternating p and 1.  Then 300 random product sets (1..7 products of values below 2p), each through the
    Karatsuba engine, the 14-limb schoolbook engine and, with X scaled by a random m < 2^12 (m X may pass 2^392),
    the 15-limb schoolbook engine."""
    cases = []
    for prods, x15, kara in op_shapes():
        for fill in ("p", "p-1", "alt"):
            seq = 0
            vals = []
            for m, nx, ny in prods:
                t = []
                for _ in range(nx + ny):
                    t.append({"p": P, "p-1": P - 1}.get(fill, P if seq % 2 == 0 else 1))
                    seq += 1
                vals.append((m * sum(t[:nx]), sum(t[nx:])))
            cases.append((vals, kara, x15))
    rng = random.Random(7)
    for _ in range(300):
        prods = [(rng.randrange(2 * P), rng.randrange(2 * P)) for _ in range(rng.randrange(1, 8))]
        cases.append((prods, True, False))
        cases.append((prods, False, False))
        cases.append(([(x * rng.randrange(1, 1 << 12), y) for x, y in prods], False, True))
    for prods, kara, x15 in cases:
        _assert_contract(prods, kara, x15)
    return cases


def check_columns(case, cols, words):
    """cols: the 28 raw 64-bit columns after the products (and the join); words: the 13 words of sop_redc28."""
    prods, kara, x15 = case
    tag = (kara, x15, [(hex(x), hex(y)) for x, y in prods])
    assert [int(c) for c in cols] == exact_columns(prods, x15), tag
    assert sum(int(w) << (32 * i) for i, w in enumerate(words)) == exact_redc(prods), tag


# ---------------------------------------------------------------------------------------------- soptest files
# (layout: tools/microbench/soptest.hip)
REDUCE_IN, REDUCE_OUT = 15, 13
C28_IN, C28_OUT = 24, 26
COL_IN, COL_OUT = 2 + KMAX * 25, 56 + 13


def _words(v, n):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def reduce_record(case):
    v, red, use_table = case
    return _words(v, 13) + [red, use_table]


def c28_record(case):
    return _words(case[0], 12) + _words(case[1], 12)


def column_record(case):
    prods, kara, x15 = case
    w = [len(prods), int(kara) | int(x15) << 1]
    for X, Y in prods:
        w += _words(X, 13) + _words(Y, 12)
    return w + [0] * (25 * (KMAX - len(prods)))


def pack_input(reduce=(), c28=(), columns=()):
    w = []
    for cases, rec, width in ((reduce, reduce_record, REDUCE_IN), (c28, c28_record, C28_IN),
                              (columns, column_record, COL_IN)):
        w.append(len(cases))
        for c in cases:
            r = rec(c)
            assert len(r) == width
            w += r
    return struct.pack("<%dI" % len(w), *w)


def unpack_output(data, n_reduce, n_c28, n_columns):
    """-> (reduce: [13 words], c28: [(mul 13 words, sqr 13 words)], columns: [(28 columns, 13 words)])"""
    assert len(data) == 4 * (n_reduce * REDUCE_OUT + n_c28 * C28_OUT + n_columns * COL_OUT)
    w = struct.unpack("<%dI" % (len(data) // 4), data)
    at = 0
    red = [w[at + REDUCE_OUT * i: at + REDUCE_OUT * (i + 1)] for i in range(n_reduce)]
    at += REDUCE_OUT * n_reduce
    c28 = [(w[at + C28_OUT * i: at + C28_OUT * i + 13], w[at + C28_OUT * i + 13: at + C28_OUT * (i + 1)])
           for i in range(n_c28)]
    at += C28_OUT * n_c28
    cols = []
    for i in range(n_columns):
        r = w[at + COL_OUT * i: at + COL_OUT * (i + 1)]
        cols.append(([r[2 * c] | r[2 * c + 1] << 32 for c in range(28)], r[56:]))
    return red, c28, cols
