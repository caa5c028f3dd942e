"""Participant sets that exercise the LAYOUT of the masked aggregation kernel (item_agg_team, csrc/lcv_items.hpp),
shared by test_aggregate_layout_hostsim.py (host simulation) and test_aggregate_layout_gpu.py (the MI355X), through
lcv_debug_aggregate (which launches F_agg_team).

The kernel gives an update to 4 lanes: lane l sums the members 128 l .. 128 l + 127 (quarter l) with mixed additions,
a two-round tree of full Jacobian additions joins the four partial sums (round 1: lanes 0+1 and 2+3; round 2:
0+2), and with more than 256 participants the lanes sum the negated NON-participants and lane 0 adds the
committee's total.  So the sets below put the special cases of the additions where the layout makes them happen:
an identity partial sum entering the tree on either side, equal points meeting in round 1 or round 2 (doubling), sums
cancelling inside a quarter, in round 1 and in round 2, the complement step ending in a doubling, in the identity and
on its `acc == identity` shortcut, participation counts around the threshold, and item counts around the 16 teams
of a wave.

Committees are made from CHOSEN secret keys, so a relation between members is set by solving for one key mod r.
Expected points and statuses come from oracle/bls12_381.py alone: every key is decompressed once and the
participants' points are added with g1_add (status 2 where an invalid key participates, 1 where the sum is the
identity, else 0).  Exact integers: equality, no tolerance.
"""
import random
from functools import lru_cache

import numpy as np

from oracle import bls12_381 as B

R = B.R
CALL_SIZES = (1, 15, 16, 17, 33)  # items per lcv_debug_aggregate call: 16 teams of 4 lanes fill a wave


def quarter(k):
    return list(range(128 * k, 128 * k + 128))


@lru_cache(maxsize=None)
def _base_table():
    """[w][d - 1] = d * 16^w * G for the 64 four-bit windows of a scalar."""
    out, p = [], B.G1_GEN
    for _ in range(64):
        row, acc = [], None
        for _ in range(15):
            acc = B.g1_add(acc, p)
            row.append(acc)
        out.append(row)
        p = B.g1_add(row[14], p)
    return out


def pubkey_point(sk: int):
    """sk * G by fixed-base windows (64 additions of the oracle's g1_add)."""
    acc = None
    for w, row in enumerate(_base_table()):
        d = (sk >> (4 * w)) & 15
        if d:
            acc = B.g1_add(acc, row[d - 1])
    return acc


def _non_subgroup_key() -> bytes:
    x = 40
    while True:
        x += 1
        y = B.fp_sqrt((x * x * x + B.B1) % B.P)
        if y is not None and not B.g1_in_subgroup((x, y)):
            return B.g1_compress((x, y))


class Table:
    """A 512-key committee table: sks (None where the key is not a valid one), compressed keys, decoded points."""

    def __init__(self, sks, bad=()):
        assert all(0 < k < R for k in sks)
        self.sks = list(sks)
        self.points = [pubkey_point(k) for k in sks]
        self.pks = [B.g1_compress(p) for p in self.points]
        for j, raw in bad:
            self.sks[j], self.points[j], self.pks[j] = None, None, raw
            assert not B.key_validate(raw)
        for j in (0, 5, 511):  # the windowed multiplication against the oracle's own
            if self.sks[j] is not None:
                assert self.pks[j] == B.sk_to_pk(self.sks[j])
                assert B.g1_decompress(self.pks[j]) == self.points[j]
        self.raw = np.frombuffer(b"".join(self.pks), np.uint8)

    def expected(self, members):
        """(status, affine sum or None) of the participants `members`, by adding their points."""
        acc = None
        for j in members:
            if self.points[j] is None:
                return 2, None
            acc = B.g1_add(acc, self.points[j])
        return (1, None) if acc is None else (0, acc)


class Layout:
    """tables: A (relations across quarters), B (relations of the complement step), C (invalid keys);
    items: (label, table index, sorted members)."""

    def __init__(self):
        everyone = list(range(512))

        def without(*gone):
            return [j for j in everyone if j not in gone]
        # ---- A: equal and cancelling members across the quarters
        rng = random.Random(41)
        a = [rng.randrange(1, R) for _ in range(512)]
        a[133] = a[261] = a[389] = a[5]          # 5 = 133 meets in round 1, 5 = 261 in round 2, 133 = 389 in round 2
        a[21] = a[20]                            # equal members inside quarter 0
        a[130] = R - a[2]                        # cancels inside round 1
        a[400] = -(a[2] + a[140] + a[270]) % R   # cancels in round 2
        items = [("A_equal_5_133", 0, [5, 133]), ("A_equal_5_261", 0, [5, 261]), ("A_equal_133_389", 0, [133, 389]),
                 ("A_equal_5_133_and_300", 0, [5, 133, 300]), ("A_equal_5_261_and_450", 0, [5, 261, 450]),
                 ("A_equal_133_389_and_50", 0, [50, 133, 389]), ("A_equal_5_133_261_389", 0, [5, 133, 261, 389]),
                 ("A_cancel_2_130", 0, [2, 130]), ("A_cancel_2_130_and_300", 0, [2, 130, 300]),
                 ("A_cancel_2_140_270_400", 0, [2, 140, 270, 400]),
                 ("A_missing_2_130_sum_to_identity", 0, without(2, 130)),
                 ("A_missing_equal_20_21_one_quarter", 0, without(20, 21)),
                 ("A_missing_equal_5_133_round_1", 0, without(5, 133)),
                 ("A_missing_equal_5_261_round_2", 0, without(5, 261)),
                 ("A_missing_2_140_270_400_sum_to_identity", 0, without(2, 140, 270, 400))]
        # ---- B: the complement step's last addition
        rng = random.Random(42)
        b = [rng.randrange(1, R) for _ in range(512)]
        zero_sum = sorted(set(rng.sample(everyone, 299)) | {7})            # > 256 participants summing to the identity
        b[7] = -sum(b[j] for j in zero_sum if j != 7) % R
        free = next(j for j in everyone if j not in zero_sum)
        doubling = sorted(set(rng.sample(everyone, 400)) | {free})          # sum_P = -2 sum_N: acc == all at the end
        rest = [j for j in everyone if j not in doubling]
        b[free] = (-2 * sum(b[j] for j in rest) - sum(b[j] for j in doubling if j != free)) % R
        assert free not in zero_sum and len(zero_sum) > 256 and len(doubling) > 256
        order = rng.sample(everyone, 512)
        items += [("B_participants_sum_to_identity", 1, zero_sum), ("B_last_addition_is_a_doubling", 1, doubling)]
        items += [(f"B_popcount_{n}", 1, sorted(order[:n])) for n in (255, 256, 257, 258)]
        items += [(f"B_popcount_511_missing_{m}", 1, without(m)) for m in (100, 200, 300, 400)]
        items += [("B_popcount_512", 1, everyone), ("B_missing_only_in_quarter_3", 1, list(range(384)) + [500]),
                  ("B_missing_only_in_quarter_1", 1, quarter(0) + [129] + quarter(2) + quarter(3))]
        # ---- C: invalid keys, missing and participating
        rng = random.Random(43)
        c = [rng.randrange(1, R) for _ in range(512)]
        bad = ((77, _non_subgroup_key()), (300, bytes([0xC0]) + bytes(47)))
        for k in range(4):  # participants in one quarter only: the other lanes' partial sums are the identity
            items.append((f"C_only_quarter_{k}", 2, sorted(rng.sample([j for j in quarter(k) if j not in (77, 300)], 40))))
        items += [("C_one_member_per_quarter", 2, [10, 200, 301, 500]),
                  ("C_quarters_0_2", 2, [11, 12, 290, 291]), ("C_quarters_1_3", 2, [150, 160, 420, 430]),
                  ("C_quarters_0_3", 2, [60, 61, 470, 471])]
        items += [("C_invalid_keys_missing", 2, without(77, 300)), ("C_invalid_key_77_participates", 2, without(300)),
                  ("C_everyone_with_invalid_keys", 2, everyone), ("C_invalid_key_in_small_set", 2, [76, 77, 78]),
                  ("C_small_set_beside_invalid_key", 2, [76, 78, 299, 301]), ("C_single_member_511", 2, [511])]
        self.tables = [Table(a), Table(b), Table(c, bad)]
        # committee_id varies from row to row: round-robin over the tables
        by_table = [[it for it in items if it[1] == t] for t in range(3)]
        self.items = []
        for k in range(max(len(x) for x in by_table)):
            self.items += [x[k] for x in by_table if k < len(x)]
        self.expected = {label: self.tables[t].expected(m) for label, t, m in self.items}
        self.committees = np.stack([t.raw for t in self.tables])

    def check_relations(self):
        """The relations the sets were built for, as the oracle sees them (so a set keeps meaning what its name says)."""
        A, Bt, _ = self.tables
        e = self.expected
        status = {k: v[0] for k, v in e.items()}
        assert A.points[5] == A.points[133] == A.points[261] == A.points[389] and A.points[20] == A.points[21]
        assert A.points[130] == B.g1_neg(A.points[2])
        for k in ("A_cancel_2_130", "A_cancel_2_140_270_400", "B_participants_sum_to_identity"):
            assert status[k] == 1, k
        assert e["A_equal_5_133"][1] == B.g1_add(A.points[5], A.points[5])
        total_a = A.expected(range(512))[1]
        assert e["A_missing_2_130_sum_to_identity"][1] == total_a == e["A_missing_2_140_270_400_sum_to_identity"][1]
        members = dict((label, m) for label, _, m in self.items)
        dbl = members["B_last_addition_is_a_doubling"]
        s_n = Bt.expected([j for j in range(512) if j not in dbl])[1]
        total_b = Bt.expected(range(512))[1]
        assert total_b == B.g1_neg(s_n) and e["B_last_addition_is_a_doubling"][1] == B.g1_add(total_b, total_b)
        assert status["C_invalid_keys_missing"] == 0 and status["C_invalid_key_77_participates"] == 2
        assert status["C_everyone_with_invalid_keys"] == 2 and status["C_invalid_key_in_small_set"] == 2
        assert set(status.values()) == {0, 1, 2}
        assert {len(m) for m in members.values()} >= {1, 2, 255, 256, 257, 258, 510, 511, 512}
        # every item is in one of the calls
        seen = set()
        for n in CALL_SIZES:
            seen |= {it[0] for it in self.call(n)}
        assert seen == set(members), set(members) - seen
        assert sum(CALL_SIZES) >= len(self.items) > 33

    def call(self, n):
        """The items of the call of size n: consecutive stretches of the (cyclic) item list."""
        start = sum(s for s in CALL_SIZES[:CALL_SIZES.index(n)])
        return [self.items[(start + t) % len(self.items)] for t in range(n)]


@lru_cache(maxsize=None)
def layout() -> Layout:
    return Layout()


def bits_of(members) -> bytes:
    b = bytearray(64)
    for j in members:
        b[j // 8] |= 1 << (j % 8)
    return bytes(b)


def check_call(verifier, n):
    """One lcv_debug_aggregate call of n items over the three tables against the oracle's sums."""
    lay = layout()
    items = lay.call(n)
    cid = np.array([t for _, t, _ in items], np.uint32)
    assert n < 3 or (set(cid.tolist()) == {0, 1, 2} and 2 * int((cid[1:] != cid[:-1]).sum()) >= n - 1)
    out, st = verifier.debug_aggregate(lay.committees, cid, np.frombuffer(b"".join(bits_of(m) for _, _, m in items), np.uint8))
    bad = []
    for i, (label, _, _) in enumerate(items):
        want_st, want = lay.expected[label]
        got = bytes(out[i])
        point = (int.from_bytes(got[:48], "big"), int.from_bytes(got[48:96], "big"))
        if int(st[i]) != want_st or (want_st == 0 and point != want):
            bad.append((i, label, int(st[i]), want_st))
    assert not bad, bad
