"""The reference at the accumulator maxima, on the CPU.  test_gpu_mac_planted.py
brings the key-switch and diagonal multiply-accumulate kernels to the bounds
of their unreduced accumulators by planting every operand -- the ciphertext
(helpers.max_digit_ct), the key words (the "max key") and the diagonals --
and compares bit for bit with the oracle.  These tests pin what that
comparison rests on before any GPU run: that the planted digits really are
t - 1 (helpers.digits_at_max), that the oracle's own u128 arithmetic is right
on 61-bit operands at their maximum (against Python integers), that the
planted positions cover at least a quarter of every attacked limb, and that
the index sets of the planted linear transforms split as the GPU tests say."""
import numpy as np
import pytest

from tests.helpers import (EDGE, EDGE_BITS, LT_IDX, MAC_CHAINS, MAC_DIGIT_CASES, bsgs_split, digit_limbs, digits_at_max,
                           expected_digits, key_mask, max_digit_ct, max_key, max_mask, neg_pinv_rows, share_at_max)

_orcs = {}


def chain_oracle(oracle_mod, name):
    if name not in _orcs:
        ch = MAC_CHAINS[name]
        _orcs[name] = oracle_mod.Oracle.from_logs(ch["logn"], ch["logq"], ch["logp"])
    return _orcs[name]


def test_edge_chain_bit_lengths(oracle_mod):
    orc = chain_oracle(oracle_mod, "edge")
    assert [q.bit_length() for q in orc.moduli] == EDGE_BITS
    bits = EDGE_BITS
    for lo, hi in ((48, 49), (52, 53), (60, 61)):  # a limb on each side of every path switch
        assert any(b <= lo for b in bits) and any(b >= hi for b in bits)
    assert 48 in bits and 49 in bits and 52 in bits and 60 in bits and 61 in bits
    for limbs in digit_limbs(7, orc.K):  # every full digit exceeds every t - 1
        assert sum(bits[j] for j in limbs) > 62


@pytest.mark.parametrize("name,level", MAC_DIGIT_CASES)
def test_digit_counts(oracle_mod, name, level):
    """every case of the GPU tests: beta digits at t - 1 on the target limb, or
    beta - 1 where the last digit is a single prime narrower than the target"""
    orc = chain_oracle(oracle_mod, name)
    beta = len(digit_limbs(level, orc.K))
    short = 0
    for target in orc.qp_mods(level):
        want = expected_digits(orc, level, target)
        assert want in (beta, beta - 1)
        short += want == beta - 1
        assert digits_at_max(orc, level, target, max_digit_ct(orc, level, target)[1]) == want, (name, level, target)
    if (name, level) == ("edge", 4):  # the 54-bit last digit: short on the 60- and 61-bit targets
        assert short == 3
    else:
        assert short == 0


def digit_rows(orc, level, c1):
    """D[i][pos]: the beta digit rows of c1 on every QP limb (NTT domain), by
    intt, modup_digit and ntt"""
    qp = orc.qp_mods(level)
    out = []
    for limbs in digit_limbs(level, orc.K):
        src = np.stack([orc.intt(j, c1[j]) for j in limbs])
        rest = [m for m in qp if m not in limbs]
        ext = orc.modup_digit(src, limbs, rest)
        rows = {m: orc.ntt(m, ext[k]) for k, m in enumerate(rest)}
        rows.update({j: c1[j] for j in limbs})
        out.append([rows[m] for m in qp])
    return out


@pytest.mark.parametrize("name,level", [("edge", 7), ("edge", 4), ("wide", 8)])
def test_oracle_gadget_product_at_maxima(oracle_mod, name, level):
    """gadget_product_lazy on a max_digit_ct image under a max key, against
    sum_i D_i key_i mod q in Python integers at 16 positions of M and 16
    outside it, on every limb; where all beta pairs are at the maximum the
    value is beta mod q ((q - 1)^2 = 1)."""
    orc = chain_oracle(oracle_mod, name)
    rng = np.random.default_rng(61 + level)
    g = orc.galois_element(1)
    M = max_mask(orc.N)
    mk = key_mask(orc, M, g)
    base = np.stack([np.stack([np.stack([rng.integers(0, q, orc.N, dtype=np.uint64) for q in orc.moduli])
                               for _ in range(2)]) for _ in range(orc.dnum)])
    key = max_key(base, orc.moduli, mk)
    pos = list(np.flatnonzero(mk)[:16]) + list(np.flatnonzero(~mk)[:16])
    qp = orc.qp_mods(level)
    beta = len(digit_limbs(level, orc.K))
    targets = qp if orc.K > 1 else [0]
    closed = 0
    for target in targets:
        c1 = max_digit_ct(orc, level, target)[1]
        u = orc.gadget_product_lazy(c1, key, level)
        D = digit_rows(orc, level, c1)
        for c in range(2):
            for p, m in enumerate(qp):
                q = orc.moduli[m]
                for n in pos:
                    want = sum(int(D[i][p][n]) * int(key[i, c, m, n]) for i in range(beta)) % q
                    assert int(u[c][p][n]) == want, (target, c, m, n)
                full = expected_digits(orc, level, m) == beta and (m == target or orc.K == 1)
                if full:  # all beta pairs at (q - 1)^2 on M
                    assert all(int(D[i][p][n]) == q - 1 for i in range(beta) for n in pos)
                    assert np.all(u[c][p][mk] == beta % q), (target, c, m)
                    closed += 1
    assert closed >= 2 * (len(qp) if orc.K == 1 else len(qp) - 3 * ((name, level) == ("edge", 4)))


@pytest.mark.parametrize("name", ["edge", "lat"])
def test_share_at_maximum(oracle_mod, name):
    """M is half of the positions; the key masks of the amounts the GPU tests
    use meet on M after their automorphisms, so a sum over all of them is at
    the maximum on |M| / N >= 1/4 of every attacked limb, and a single
    rotation or diagonal product on the same share"""
    orc = chain_oracle(oracle_mod, name)
    M = max_mask(orc.N)
    assert 0.25 <= M.mean() <= 0.75
    gels = [orc.galois_element(k) for k in list(range(1, 18)) + [-4, 300]]
    masks = {g: key_mask(orc, M, g) for g in gels}
    for g in gels:
        assert masks[g].sum() == M.sum()
        assert share_at_max(orc, {g: masks[g]}) == M.mean() >= 0.25
    assert not np.array_equal(masks[gels[0]], masks[gels[1]])
    assert share_at_max(orc, masks) == M.mean() >= 0.25
    # the t0 addend P c0 of a rotation sum is q_j - 1 everywhere under c0 = -P^-1
    P = 1
    for k in range(orc.K):
        P *= orc.moduli[orc.L + k]
    for j, r in enumerate(neg_pinv_rows(orc, orc.L - 1)):
        assert P * r % orc.moduli[j] == orc.moduli[j] - 1


@pytest.mark.parametrize("which,n1", [("lt8", 8), ("lt16", 16)])
def test_planted_transform_index_sets(oracle_mod, which, n1):
    """the planted transforms: N1 = 8 and 16 under LogBabyStepGiantStepRatio 1,
    no s = 0 baby, and a fullest giant with all N1 - 1 babies (7 of the
    8-slot kernels' slots, 15 of the 16-slot kernels')"""
    orc = chain_oracle(oracle_mod, "edge")
    idx = LT_IDX[which]
    assert orc.find_best_bsgs_n1(idx, 1) == n1
    split = [bsgs_split(d, orc.slots, n1) for d in idx]
    assert all(b != 0 for _, b in split)
    per = {}
    for gi, b in split:
        per.setdefault(gi, set()).add(b)
    assert max(len(v) for v in per.values()) == n1 - 1 == len({b for _, b in split})
    assert len(per) > 1
