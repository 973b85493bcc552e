"""The identities slot-packed bootstrapping rests on (CPU oracle only; include/orion_hip.h,
OrionHipPackMonomials .. OrionHipBootstrapMany):

  - the NTT of X^k is psi^(k (2 brv(j) + 1)) at coefficient j, k taken mod 2N with X^(N + k) = -X^k;
  - on plaintext polynomials, unpack o pack followed by the sum over the automorphisms sigma_(5^(n j)),
    n = N / (2 g), is g times the projection of each image onto Z[X^g], every other image of its group killed
    exactly -- a ragged last group included;
  - the composed path (mean trace at level 0, pack, full-slot bootstrap, unpack, sum trace at the top) on the
    oracle's own circuit and keys refreshes every image of a ragged group of three.

These tests use the oracle alone: they pin the construction, not the library's code, and pass with or without
the feature (tests/test_btp_many_api.py and tests/test_gpu_btp_many.py are the ones that need it)."""
import numpy as np
import pytest

from tests.slot_pack_helpers import brv, btp_test_keys, mono, pack, unit, unpack  # noqa: F401

LOGNS = [10, 11, 12, 13]


@pytest.mark.parametrize("logn", LOGNS)
def test_ntt_of_a_monomial_is_a_power_of_psi(oracle_mod, logn):
    orc = oracle_mod.Oracle.from_logs(logn, [60, 40], [61])
    N = orc.N
    odd = [2 * brv(j, logn) + 1 for j in range(N)]
    for g in (2, 8):
        for k in (1, g - 1, N - 1, N, 2 * N - 1):
            for m in range(2):
                q, psi = orc.moduli[m], orc.psi(m)
                exp = np.array([pow(psi, k * e % (2 * N), q) for e in odd], dtype=np.uint64)
                assert np.array_equal(orc.ntt(m, unit(N, k, q)), exp), (g, k, m)


@pytest.mark.parametrize("logn", LOGNS)
@pytest.mark.parametrize("g,B", [(2, 3), (8, 8), (8, 11)])
def test_unpack_of_pack_then_the_trace_is_g_times_the_projection(oracle_mod, logn, g, B):
    orc = oracle_mod.Oracle.from_logs(logn, [60, 40], [61])
    N, nl = orc.N, 2
    n = N // (2 * g)
    rng = np.random.default_rng(100 * logn + g + B)
    q = np.array(orc.moduli[:nl], dtype=np.uint64)[:, None]
    coeff = np.stack([np.stack([rng.integers(0, orc.moduli[j], N, dtype=np.uint64) for j in range(nl)])
                      for _ in range(B)])  # B dense images, coefficient domain
    proj = coeff.copy()
    proj[:, :, np.arange(N) % g != 0] = 0  # the projection onto Z[X^g]
    x = np.stack([np.stack([orc.ntt(j, proj[b, j]) for j in range(nl)]) for b in range(B)])
    y = pack(orc, x, g)
    assert y.shape[0] == -(-B // g)
    w = unpack(orc, y, g, B)
    for b in range(B):
        t = w[b]
        for s in range(g.bit_length() - 1):  # t += sigma_(5^(n 2^s)) t
            t = (t + orc.automorphism_ntt(t, orc.galois_element(n << s))) % q
        got = np.stack([orc.intt(j, t[j]) for j in range(nl)])
        exp = np.stack([proj[b, j].astype(object) * g % orc.moduli[j] for j in range(nl)]).astype(np.uint64)
        assert np.array_equal(got, exp), b
    # the trace alone on a dense image: g times its projection
    d = np.stack([orc.ntt(j, coeff[0, j]) for j in range(nl)])
    for s in range(g.bit_length() - 1):
        d = (d + orc.automorphism_ntt(d, orc.galois_element(n << s))) % q
    got = np.stack([orc.intt(j, d[j]) for j in range(nl)])
    exp = np.stack([proj[0, j].astype(object) * g % orc.moduli[j] for j in range(nl)]).astype(np.uint64)
    assert np.array_equal(got, exp)


def test_oracle_bootstrap_many_functional(oracle_mod):
    """The composed path on the oracle alone, in the setting of test_oracle_bootstrap_functional (N = 2^13,
    [60] + [40] x 5, P [61, 61], h = 192, keys made by the oracle): three images with N/16 slots (g = 8, one
    ragged group) -- mean trace at level 0, pack, one full-slot Oracle.bootstrap, unpack and sum trace at the
    top level -- every image decrypted against its cleartext, replicated.  Bar: that test's own, max error
    < 1e-7 (measured per image 4.5e-8, 6.7e-8, 4.9e-8)."""
    logq, logp = [60] + [40] * 5, [60, 60]
    sm = oracle_mod.gen_moduli(13, logq, logp)
    bq, bp = oracle_mod.btp_chain(13, sm, len(logq), [61, 61])
    boot = oracle_mod.Oracle(13, bq + bp, len(bq), len(bp))
    sc = oracle_mod.Oracle(13, sm, len(logq), len(logp))
    N, n, top = boot.N, boot.N // 2, len(logq) - 1
    g, B = 8, 3
    ns = n // g
    circ = oracle_mod.BtpCircuit(boot, 40, n)
    sk = boot.gen_secret(7, 192)
    keys = btp_test_keys(boot, sk, circ, 50)
    steps = [boot.galois_element(ns << s) for s in range(g.bit_length() - 1)]
    tk = {ge: boot.gen_evk(900 + i, sk, boot.automorphism_ntt(sk, pow(ge, -1, 2 * N))) for i, ge in enumerate(steps)}
    rng = np.random.default_rng(6)
    vals = rng.uniform(-1, 1, (B, n))
    vals[:, ns:] = 0

    def trace(ct, level, mean):
        q = np.array(boot.moduli[:level + 1], dtype=np.uint64)[:, None]
        if mean:
            ct = np.stack([np.stack([ct[c, j].astype(object) * pow(g, -1, boot.moduli[j]) % boot.moduli[j]
                                     for j in range(level + 1)]) for c in range(2)]).astype(np.uint64)
        for ge in steps:
            ct = (ct + boot.rotate(ct, ge, tk[ge], level)) % q
        return ct

    x = np.stack([boot.encrypt_sk(3 + b, sk, boot.encode(vals[b], 2.0 ** 40, [0]), 0) for b in range(B)])
    u = np.stack([trace(x[b], 0, True) for b in range(B)])
    p = pack(boot, u, g)
    assert p.shape[0] == 1
    r, osc = sc.bootstrap(boot, circ, keys, p[0], 0, 2.0 ** 40)
    assert osc == np.longdouble(2.0 ** 40)
    w = unpack(boot, r[None], g, B)
    errs = []
    for b in range(B):
        out = trace(w[b], top, False)
        dec = boot.decode(boot.decrypt(out, sk, top), top, 2.0 ** 40)
        errs.append(float(np.abs(dec - np.tile(vals[b, :ns], g)).max()))
    print("oracle bootstrap_many max |error| per image:", ["%.3g" % e for e in errs])
    assert max(errs) < 1e-7, errs
