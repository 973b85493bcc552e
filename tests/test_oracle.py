"""CPU tests: pin the parity oracle (oracle/ckks_oracle.c) against the
first-principles big-integer KATs in tests/golden/kat_ckks.json, and check
the CKKS-level behaviour the reference relies on.  No GPU needed."""
import json
import os

import numpy as np
import pytest

from tests.helpers import (EMBED_TOL, PLANT_CHAINS, SPLIT_CHAIN, canonical_slots, constant_rows, decode_edge_values,
                           digit_limbs, embedding_plaintext, embedding_slots, encode_planted_cases, fixed_point_rule,
                           fixed_point_y, plant_digit_values, planted_batches)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(GOLD, "kat_ckks.json")) as f:
        return json.load(f)


def test_prime_chains(kat, oracle_mod):
    for case in kat["primes"]:
        got = oracle_mod.gen_moduli(case["logn"], case["logq"], case["logp"])
        assert got == case["moduli"]
        nth = 2 << case["logn"]
        for q, b in zip(got, case["logq"] + case["logp"]):
            assert q % nth == 1
            assert abs(np.log2(q) - b) < 0.5


def test_primitive_root(kat, oracle_mod):
    for c in kat["ntt"]:
        assert oracle_mod.lib().oracle_primitive_root(c["q"]) == c["g"]


def test_ntt_definition(kat, oracle_mod):
    for c in kat["ntt"]:
        o = oracle_mod.Oracle(c["logn"], [c["q"]], 1, 0)
        assert o.psi(0) == c["psi"]
        a = np.array(c["a"], dtype=np.uint64)
        assert [int(x) for x in o.ntt(0, a)] == c["out"]
        assert np.array_equal(o.intt(0, o.ntt(0, a)), a)


def _chain(kat, oracle_mod):
    ch = kat["chain"]
    return oracle_mod.Oracle(ch["logn"], ch["moduli"], ch["L"], ch["K"])


def test_basis_extension_exact(kat, oracle_mod):
    o = _chain(kat, oracle_mod)
    c = kat["basisext"]
    got = o.basis_extend(np.array(c["x"], dtype=np.uint64), c["src"], c["dst"])
    assert got.tolist() == c["out"]
    # the float64 quotient: Lattigo's division form, on coefficients where it
    # differs from floor(x / S) and from a reciprocal multiply
    for c in kat["bext_quotient"]:
        assert any(a != b for a, b in zip(c["v_div"], c["v_rcp"]))
        assert any(a != b for a, b in zip(c["v_div"], c["v_floor"]))
        got = o.basis_extend(np.array(c["x"], dtype=np.uint64), c["src"], c["dst"])
        assert got.tolist() == c["out"], c["src"]


def test_modup_single_prime_digit_centered(kat, oracle_mod):
    """DecomposeAndSplit's single-prime digit extends x - s for x >= s >> 1"""
    o = _chain(kat, oracle_mod)
    c = kat["modup_single"]
    got = o.modup_digit(np.array(c["x"], dtype=np.uint64), c["src"], c["dst"])
    assert got.tolist() == c["out"]
    # wider digits: the same as ModUpExact
    c = kat["bext_quotient"][0]
    x = np.array(c["x"], dtype=np.uint64)
    assert np.array_equal(o.modup_digit(x, c["src"], c["dst"]), o.basis_extend(x, c["src"], c["dst"]))


def test_rescale_round(kat, oracle_mod):
    o = _chain(kat, oracle_mod)
    c = kat["rescale"]
    lvl = c["level"]
    x = np.array(c["x"], dtype=np.uint64)
    xn = np.stack([o.ntt(j, x[j]) for j in range(lvl + 1)])
    out = o.rescale(np.stack([xn, xn]), lvl)
    for comp in range(2):
        coef = [o.intt(j, out[comp, j]).tolist() for j in range(lvl)]
        assert coef == c["out"]


def test_moddown_floor(kat, oracle_mod):
    o = _chain(kat, oracle_mod)
    c = kat["moddown"]
    lvl = c["level"]
    x = np.array(c["x"], dtype=np.uint64)
    mods = o.qp_mods(lvl)
    xn = np.stack([o.ntt(m, x[j]) for j, m in enumerate(mods)])
    out = o.moddown(xn, lvl)
    coef = [o.intt(j, out[j]).tolist() for j in range(lvl + 1)]
    assert coef == c["out"]


def test_automorphism_ntt_domain(kat, oracle_mod):
    o = _chain(kat, oracle_mod)
    c = kat["automorph"]
    m = c["modidx"]
    a = np.array(c["a"], dtype=np.uint64)
    an = o.ntt(m, a)[None]
    for case in c["cases"]:
        # the oracle permutes all limbs with moduli index 0..; use a 1-limb chain for modidx
        o1 = oracle_mod.Oracle(kat["chain"]["logn"], [o.moduli[m]], 1, 0)
        got = o1.automorphism_ntt(o1.ntt(0, a)[None], case["g"])
        assert o1.intt(0, got[0]).tolist() == case["out"]
    assert an.shape[0] == 1


def test_galois_elements(oracle_mod):
    o = oracle_mod.Oracle.from_logs(13, [50, 40], [60])
    M = 2 * o.N
    assert o.galois_element(0) == 1
    assert o.galois_element(1) == 5
    assert o.galois_element(-1) == pow(5, o.N // 2 - 1, M)
    assert o.galois_element(o.N // 2) == 1  # 5 has order N/2 mod 2N


def test_bsgs_ratio_lola_shapes(oracle_mod):
    """FindBestBSGSRatio with LogBSGSRatio = int(ln 2) = 0 (lineartransform.go:67)."""
    o = oracle_mod.Oracle.from_logs(15, [60, 40], [60])
    assert o.find_best_bsgs_n1(list(range(128)), 0) == 8
    conv = [0, 1, 27, 28, 29, 1264, 1265, 1292, 1293, 2019, 2020, 2021, 2047]
    n1 = o.find_best_bsgs_n1(conv, 0)
    assert n1 >= 1 and (n1 & (n1 - 1)) == 0


@pytest.fixture(scope="module")
def ckks(oracle_mod):
    o = oracle_mod.Oracle.from_logs(12, [55, 40, 40, 40, 40], [60, 60])
    sk = o.gen_secret(5, 64)
    return o, sk


def test_encode_decode_roundtrip(ckks):
    o, _ = ckks
    rng = np.random.default_rng(0)
    v = rng.uniform(-3, 3, o.N // 2)
    pt = o.encode(v, 2.0 ** 40, list(range(5)))
    assert np.abs(o.decode(pt, 4, 2.0 ** 40) - v).max() < 1e-7


def test_encode_big_values_exact(ckks):
    """|v * scale| >= 2^64 takes Lattigo's exact big-integer path: the residues
    are those of the integer v * scale (a double, so mant * 2^e exactly)."""
    o, _ = ckks
    from fractions import Fraction
    n = o.N // 2
    v = np.zeros(n)
    v[0] = 3.0
    scale = 2.0 ** 70
    pt = o.encode(v, scale, list(range(5)))
    # slot constant 3 at slot 0 only -> check through the decode round trip
    assert abs(o.decode(pt, 4, scale)[0] - 3.0) < 1e-9
    # a direct check of the reduction: every coefficient as an exact integer
    coef = o.intt(0, pt[0].copy())
    assert coef.dtype == np.uint64 and np.any(coef != 0)


def test_chacha20_rfc8439_block(oracle_mod):
    """RFC 8439 §2.3.2 test vector (key 00..1f, counter 1, nonce 00 00 00 09
    00 00 00 4a 00 00 00 00): the encryption sampler's block function."""
    key = np.frombuffer(bytes(range(32)), dtype="<u4").copy()
    nonce = np.frombuffer(bytes([0, 0, 0, 9, 0, 0, 0, 0x4A, 0, 0, 0, 0]), dtype="<u4").copy()
    out = oracle_mod.chacha20_block(key, 1, nonce)
    exp = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
           0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]
    assert [int(x) for x in out] == exp


def test_gauss_cdt_table(oracle_mod):
    """t[i] = floor(2^64 P(X <= -19 + i)) for the discrete Gaussian sigma 3.2
    on |x| <= 19, checked against exact rational arithmetic of the same
    float64 weights."""
    from fractions import Fraction
    import math
    t = oracle_mod.gauss_cdt(3.2, 19)
    rho = [math.exp(-(x * x) / (2.0 * 3.2 * 3.2)) for x in range(-19, 20)]
    tot = sum(Fraction(r) for r in rho)
    acc = Fraction(0)
    for i in range(38):
        acc += Fraction(rho[i])
        exact = int(acc / tot * 2 ** 64)
        assert abs(int(t[i]) - exact) <= 2 ** 12, i  # float64 rounding of the cumulative sum
    assert np.all(np.diff(t.astype(object)) > 0)


def test_encryption_sampler_statistics(oracle_mod):
    N = 1 << 15
    u = oracle_mod.enc_sample(N, 77, 0, 0, 0)
    cnt = np.bincount(u + 1, minlength=3)
    assert u.min() == -1 and u.max() == 1
    assert np.all(np.abs(cnt / N - 1 / 3) < 0.01)
    e = np.concatenate([oracle_mod.enc_sample(N, 77, k, b, 1 + (k & 1)) for k in range(2) for b in range(2)])
    assert np.abs(e).max() <= 19
    assert abs(e.mean()) < 0.05 and abs(e.std() - 3.2) < 0.05
    # distinct streams per (encryption, image, component)
    assert not np.array_equal(oracle_mod.enc_sample(N, 77, 0, 0, 1), oracle_mod.enc_sample(N, 77, 0, 1, 1))
    assert not np.array_equal(oracle_mod.enc_sample(N, 77, 0, 0, 1), oracle_mod.enc_sample(N, 77, 1, 0, 1))
    assert not np.array_equal(oracle_mod.enc_sample(N, 77, 0, 0, 1), oracle_mod.enc_sample(N, 77, 0, 0, 2))


def test_encrypt_pk_decrypts(ckks):
    """The restated public-key encryption decrypts to the plaintext."""
    o, sk = ckks
    N, lvl = o.N, 4
    # pk = (-a s + e, a) over QP
    rng = np.random.default_rng(3)
    LK = o.L + o.K
    a = np.stack([rng.integers(0, o.moduli[m], N, dtype=np.uint64) for m in range(LK)])
    pk = np.zeros((2, LK, N), dtype=np.uint64)
    pk[1] = a
    for m in range(LK):
        pk[0, m] = o.mul_coeffs(a[m:m + 1], sk[m:m + 1], [m])[0]
        pk[0, m] = (o.moduli[m] - pk[0, m]) % np.uint64(o.moduli[m])
    v = rng.uniform(-1, 1, N // 2)
    pt = o.encode(v, 2.0 ** 40, list(range(lvl + 1)))
    ct = o.encrypt_pk(11, 0, 0, pk, pt, lvl)
    dec = o.decode(o.decrypt(ct, sk, lvl), lvl, 2.0 ** 40)
    assert np.abs(dec - v).max() < 1e-4


@pytest.mark.parametrize("cheb,deg", [(True, 7), (True, 12), (True, 15), (False, 5), (False, 15), (False, 1)])
def test_eval_poly_functional(ckks, cheb, deg):
    """The polynomial-evaluation restatement decrypts to p(x), consumes
    bitlen(deg) levels and lands on the target scale exactly."""
    o, sk = ckks
    rng = np.random.default_rng(20 + deg)
    v = rng.uniform(-1, 1, o.N // 2)
    lvl = 4
    ct = o.encrypt_sk(21, sk, o.encode(v, 2.0 ** 40, list(range(lvl + 1))), lvl)
    rlk = o.gen_evk(4, o.mul_coeffs(sk, sk, list(range(o.L + o.K))), sk)
    cf = rng.uniform(-0.5, 0.5, deg + 1).astype(np.float32).astype(np.float64)
    out, lv, sc = o.eval_poly(ct, lvl, 2.0 ** 40, cf, cheb, 2.0 ** 40, rlk)
    assert lv == lvl - int(deg).bit_length() and sc == 2.0 ** 40
    dec = o.decode(o.decrypt(out, sk, lv), lv, 2.0 ** 40)
    exp = np.polynomial.chebyshev.chebval(v, cf) if cheb else np.polynomial.polynomial.polyval(v, cf)
    assert np.abs(dec - exp).max() < 1e-4


@pytest.mark.parametrize("cheb,deg", [(True, 63), (True, 27), (False, 40)])
def test_eval_poly_deep_functional(oracle_mod, cheb, deg):
    """Deeper Paterson-Stockmeyer trees on the CPU (recursePS: degree 63 has
    logSplit 3 and re-splits its lead node of degree 7 with logSplit 1):
    decrypts to p(x), consumes bitlen(deg) levels, exact target scale."""
    o = oracle_mod.Oracle.from_logs(12, [55] + [45] * 8, [60, 60])
    sk = o.gen_secret(6, 64)
    rng = np.random.default_rng(deg)
    v = rng.uniform(-1, 1, o.N // 2)
    lvl = 8
    ct = o.encrypt_sk(22, sk, o.encode(v, 2.0 ** 45, list(range(lvl + 1))), lvl)
    rlk = o.gen_evk(8, o.mul_coeffs(sk, sk, list(range(o.L + o.K))), sk)
    cf = (rng.uniform(-1, 1, deg + 1) / (1 + np.arange(deg + 1))).astype(np.float32).astype(np.float64)
    if deg == 27:
        cf[0::2] = 0  # odd, as a minimax sign stage
    out, lv, sc = o.eval_poly(ct, lvl, 2.0 ** 45, cf, cheb, 2.0 ** 45, rlk)
    assert lv == lvl - int(deg).bit_length() and sc == 2.0 ** 45
    dec = o.decode(o.decrypt(out, sk, lv), lv, 2.0 ** 45)
    exp = np.polynomial.chebyshev.chebval(v, cf) if cheb else np.polynomial.polynomial.polyval(v, cf)
    assert np.abs(dec - exp).max() < 1e-4


def test_encode_matches_canonical_embedding(ckks):
    """Encoding by definition: slot j = m(zeta^(5^j)), zeta = exp(i*pi/N)."""
    o, _ = ckks
    n, N = o.N // 2, o.N
    rng = np.random.default_rng(1)
    v = rng.uniform(-1, 1, n)
    pt = o.encode(v, 2.0 ** 30, [0])
    coef = o.intt(0, pt[0]).astype(np.int64)
    q = o.moduli[0]
    coef = np.where(coef > q // 2, coef - q, coef).astype(np.float64) / 2.0 ** 30
    j = np.arange(n)
    exps = np.array([pow(5, int(k), 2 * N) for k in j])
    zeta = np.exp(1j * np.pi * exps / N)
    slots = np.array([np.polyval(coef[::-1], z) for z in zeta[:64]])
    assert np.abs(slots.real - v[:64]).max() < 1e-6
    assert np.abs(slots.imag).max() < 1e-6


def test_keyswitch_relin_rotate(ckks):
    o, sk = ckks
    rng = np.random.default_rng(2)
    v = rng.uniform(-1, 1, o.N // 2)
    lvl = 4
    ct = o.encrypt_sk(3, sk, o.encode(v, 2.0 ** 40, list(range(lvl + 1))), lvl)
    rlk = o.gen_evk(4, o.mul_coeffs(sk, sk, list(range(o.L + o.K))), sk)
    sq = o.rescale(o.mul_relin(ct, ct, rlk, lvl), lvl)
    dec = o.decode(o.decrypt(sq, sk, lvl - 1), lvl - 1, 2.0 ** 80 / o.moduli[lvl])
    assert np.abs(dec - v * v).max() < 1e-5
    for k in (1, 3, -2):
        g = o.galois_element(k)
        gk = o.gen_evk(10 + k, sk, o.automorphism_ntt(sk, pow(g, -1, 2 * o.N)))
        r = o.rotate(ct, g, gk, lvl)
        dec = o.decode(o.decrypt(r, sk, lvl), lvl, 2.0 ** 40)
        assert np.abs(dec - np.roll(v, -k)).max() < 1e-5


def test_linear_transform_functional(ckks):
    o, sk = ckks
    rng = np.random.default_rng(3)
    slots = o.N // 2
    lvl = 3
    idx = [0, 1, 2, 7, 40, 41, slots - 1]
    diags = rng.uniform(-1, 1, (len(idx), slots))
    N1 = o.find_best_bsgs_n1(idx, 0)
    pts, gk = [], {}
    for i, d in enumerate(idx):
        giant = ((d // N1) * N1) % slots
        pts.append(o.encode(np.roll(diags[i], giant), float(o.moduli[lvl]), o.qp_mods(lvl)))
        for r in {giant, d % N1}:
            g = o.galois_element(r)
            if g not in gk:
                gk[g] = o.gen_evk(100 + len(gk), sk, o.automorphism_ntt(sk, pow(g, -1, 2 * o.N)))
    v = rng.uniform(-1, 1, slots)
    ct = o.encrypt_sk(9, sk, o.encode(v, 2.0 ** 40, list(range(lvl + 1))), lvl)
    y = o.rescale(o.lt_bsgs(ct, lvl, idx, pts, N1, gk), lvl)
    dec = o.decode(o.decrypt(y, sk, lvl - 1), lvl - 1, 2.0 ** 40 * o.moduli[lvl] / o.moduli[lvl])
    exp = sum(diags[i] * np.roll(v, -d) for i, d in enumerate(idx))
    assert np.abs(dec - exp).max() < 1e-5


def test_cpu_replay_lola_matches_cleartext():
    """Reference numeric gate (tests/models/test_mlp.py:45-48): the CPU oracle
    replaying the reference frontend's LoLA op stream decrypts to the
    cleartext model output within MAE 0.005."""
    from oracle.replay_cpu import CpuStream
    s = CpuStream("lola_n13")
    s.keygen()
    s.compile()
    out = s.forward(s.encrypt(s.arrays["input"]))
    v = s.decrypt(out)[:10]
    exp = s.arrays["expected_output"].reshape(-1)
    assert np.abs(v - exp).mean() < 0.005


def test_cpu_replay_mlp_conjugate_invariant():
    """tests/configs/mlp.yml as written (RingType ConjugateInvariant, 8192 real
    slots): the oracle replays the frontend's op stream on the native degree-N
    CI ring (N coefficients per limb, NthRoot 4N) and meets the reference MAE
    gate (test_mlp.py:45-48)."""
    from oracle.replay_cpu import CpuStream
    s = CpuStream("mlp_n13_ci")
    assert s.N == 1 << 13 and s.slots == 1 << 13 and s.orc.ci
    s.keygen()
    s.compile()
    out = s.forward(s.encrypt(s.arrays["input"]))
    v = s.decrypt(out)[:10]
    exp = s.arrays["expected_output"].reshape(-1)
    assert np.abs(v - exp).mean() < 0.005


def test_ci_ring_is_the_fixed_subring(oracle_mod):
    """Pins the native ConjugateInvariant ring (scheme.go:49-52) to the
    Standard ring of degree 2N (itself pinned by the big-integer KATs): for a
    CI element a (N coefficients) with expansion p (p_j = a_j, p_N = 0,
    p_{2N-j} = -a_j), the CI NTT is the first half of the 2N NTT of p, the
    CI automorphism by 5^k is the first half of the 2N one, and the CI
    encoding is the first half of the 2N encoding of the same real slots."""
    logn = 11
    mods = oracle_mod.gen_moduli(logn + 1, [40, 50, 60], [61])
    ci = oracle_mod.Oracle(logn, mods, 3, 1, ci=True)
    st = oracle_mod.Oracle(logn + 1, mods, 3, 1)
    for q in mods:
        assert q % (4 << logn) == 1  # NthRoot 4N
    N = 1 << logn
    rng = np.random.default_rng(5)
    for m in range(4):
        q = mods[m]
        a = rng.integers(0, q, N, dtype=np.uint64)
        p = np.zeros(2 * N, dtype=np.uint64)
        p[:N] = a
        p[N + 1:] = [(q - int(x)) % q for x in a[1:][::-1]]
        ref = st.ntt(m, p)
        got = ci.ntt(m, a)
        assert np.array_equal(got, ref[:N]), m
        assert np.array_equal(ci.intt(m, got), a)
        for k in (1, 7, -3):
            g = ci.galois_element(k)
            assert g == st.galois_element(k) and g % 4 == 1
            assert np.array_equal(ci.automorphism_ntt(got[None], g)[0], st.automorphism_ntt(ref[None], g)[0][:N])
    v = rng.uniform(-1, 1, N)
    pe = ci.encode(v, 2.0 ** 40, [0, 1])
    assert np.array_equal(pe, st.encode(v, 2.0 ** 40, [0, 1])[:, :N])
    assert np.abs(ci.decode(pe, 1, 2.0 ** 40) - v).max() < 1e-8


def test_cpu_replay_lola_conjugate_invariant():
    """configs/lola.yml as written (ConjugateInvariant, N=2^13): the oracle's
    native CI ring replays the frontend's op stream within the MAE gate."""
    from oracle.replay_cpu import CpuStream
    s = CpuStream("lola_n13_ci")
    assert s.orc.ci and s.slots == s.N
    s.keygen()
    s.compile()
    out = s.forward(s.encrypt(s.arrays["input"]))
    v = s.decrypt(out)[:10]
    exp = s.arrays["expected_output"].reshape(-1)
    assert np.abs(v - exp).mean() < 0.005


def test_cpu_replay_mlp_n13_c1():
    """BASELINE config C1 (configs/mlp.yml: MLP, N=2^13, [29]+[26]x5 / [29,29],
    Standard ring here, h=8192) on the CPU backend: the oracle replays the
    frontend's op stream and meets the reference MAE gate (test_mlp.py:45-48)."""
    from oracle.replay_cpu import CpuStream
    s = CpuStream("mlp_n13")
    assert s.N == 1 << 13
    s.keygen()
    s.compile()
    out = s.forward(s.encrypt(s.arrays["input"]))
    v = s.decrypt(out)[:10]
    exp = s.arrays["expected_output"].reshape(-1)
    assert np.abs(v - exp).mean() < 0.005


# ---- bootstrapping: the oracle's own circuit (Lattigo v6 defaults [U]) ----

def test_btp_cos_matches_mpmath(oracle_mod):
    """EvalMod's cosine polynomial (oracle_btp_cos: Lattigo's default
    CosDiscrete [U], binary128 Newton form rounded to 80 bits): (2 pi)^(-1/8)
    cos(2 pi (x - 1/4) / 8) interpolated at the integers -15..15, degree 30,
    equals the 60-digit mpmath solve of the interpolation system
    (tools/gen_btp_cos.py -> tests/golden/btp_cos.json) to 1e-19 per
    coefficient (measured 9e-21, the 80-bit rounding); near the small
    integers, where the ModRaise overflow lives, it is far more precise than
    a Chebyshev-node interpolant."""
    with open(os.path.join(GOLD, "btp_cos.json")) as f:
        g = json.load(f)
    c = oracle_mod.btp_cos(g["K"], g["degree"], g["r"])
    ref = np.array([np.longdouble(v) for v in g["coeffs"]], dtype=np.longdouble)  # parsed at 80 bits
    assert np.abs(c - ref).max() < 1e-19
    # within 2^-8 of every integer: 1.4e-8 at the edges |i| = 15, 5e-15 for |i| <= 8
    assert float(g["max_abs_error_on_grid"]) < 5e-8
    assert float(g["max_abs_error_near_integers_up_to_8"]) < 1e-14


def test_btp_chain_and_constants(oracle_mod):
    """The bootstrapping chain and constants the oracle derives from the
    parameters alone: residual Q kept, 3 x 39 + 8 x 60 + 4 x 56-bit circuit
    primes (Lattigo's default StC / EvalMod / CtS log-scales [U]) plus P of
    logP, none reused from the residual parameters; F = round(q0 / 2^(8 +
    logScale)); the EvalMod scale reaches 2^60 after the double angles; 4 +
    3 transforms at the right levels."""
    logq, logp = [60] + [40] * 5, [60, 60]
    sm = oracle_mod.gen_moduli(13, logq, logp)
    bq, bp = oracle_mod.btp_chain(13, sm, len(logq), [61, 61])
    assert bq[:len(logq)] == sm[:len(logq)] and len(bq) == len(logq) + 15
    sizes = [39] * 3 + [60] * 8 + [56] * 4 + [61, 61]  # primes within half a bit of 2^size
    assert all(abs(np.log2(float(q)) - b) < 0.5 for q, b in zip(bq[len(logq):] + bp, sizes))
    assert len(set(bq + bp + sm)) == len(bq) + len(bp) + len(sm) - len(logq)
    assert all(q % (2 << 13) == 1 for q in bq + bp)
    boot = oracle_mod.Oracle(13, bq + bp, len(bq), len(bp))
    for ns in (4096, 512, 2):
        c = oracle_mod.BtpCircuit(boot, 40, ns)
        p = c.params()
        assert int(p["F"]) == round(bq[0] / 2 ** 48) and int(p["K"]) == 16 and int(p["degree"]) == 30
        assert int(p["gap"]) == 4096 // ns and int(p["ntrace"]) == (4096 // ns).bit_length() - 1
        assert abs(float(p["s_y"]) / 2 ** 60 - 1) < 1e-15
        levels = [c.lt(k)[0] for k in range(7)]
        top = len(bq) - 1
        assert levels == [top, top - 1, top - 2, top - 3, top - 12, top - 13, top - 14]


def _btp_keys(o, sk, circ, seed):
    """Test keys for the oracle's circuit: relinearisation, every Galois key the
    circuit uses (BSGS babies / giants, trace, conjugation), and the ephemeral
    secret's two switching keys."""
    N, n = o.N, o.N // 2
    gels = {2 * N - 1}
    p = circ.params()
    gels |= {o.galois_element(int(p["slots"]) << i) for i in range(int(p["ntrace"]))}
    for k in range(int(p["nlt"])):
        _, n1, idx, _ = circ.lt(k)
        for d in idx:
            giant, baby = ((d // n1) * n1) % n, d % n1
            gels |= {o.galois_element(r) for r in (giant, baby) if r}
    keys = dict(rlk=o.gen_evk(seed, o.mul_coeffs(sk, sk, list(range(o.L + o.K))), sk), gks={})
    for i, g in enumerate(sorted(gels)):
        keys["gks"][g] = o.gen_evk(seed + 1 + i, sk, o.automorphism_ntt(sk, pow(g, -1, 2 * N)))
    se = o.gen_secret(seed + 999, 32)
    keys["d2s"] = o.gen_evk(seed + 1000, sk, se)
    keys["s2d"] = o.gen_evk(seed + 1001, se, sk)
    return keys


@pytest.mark.parametrize("sparse", [True, False])
def test_oracle_bootstrap_functional(oracle_mod, sparse):
    """The oracle's bootstrapping circuit works on its own, with keys the
    oracle made (no GPU, nothing from the library): a level-0 encryption
    under a dense h = 192 secret comes back on the residual top level at its
    scale, decrypting to the input (sparse slots: replicated) within 1e-7
    (CosDiscrete EvalMod; the Chebyshev-node interpolant of earlier rounds
    gave 1e-5)."""
    logq, logp = [60] + [40] * 5, [60, 60]
    sm = oracle_mod.gen_moduli(13, logq, logp)
    bq, bp = oracle_mod.btp_chain(13, sm, len(logq), [61, 61])
    boot = oracle_mod.Oracle(13, bq + bp, len(bq), len(bp))
    sc = oracle_mod.Oracle(13, sm, len(logq), len(logp))
    n = boot.N // 2
    ns = n // 8 if sparse else n
    circ = oracle_mod.BtpCircuit(boot, 40, ns)
    sk = boot.gen_secret(7, 192)
    keys = _btp_keys(boot, sk, circ, 50)
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, n)
    v[ns:] = 0
    ct = boot.encrypt_sk(3, sk, boot.encode(v, 2.0 ** 40, [0]), 0)
    out, osc = sc.bootstrap(boot, circ, keys, ct, 0, 2.0 ** 40)
    assert osc == np.longdouble(2.0 ** 40)  # the default scale comes back exactly
    top = len(logq) - 1
    dec = boot.decode(boot.decrypt(out, sk, top), top, 2.0 ** 40)
    exp = np.tile(v[:ns], n // ns)
    err = np.abs(dec - exp)
    print("oracle bootstrap error max %.3g mean %.3g" % (err.max(), err.mean()))
    assert err.max() < 1e-7 and err.mean() < 2e-8, (err.max(), err.mean())  # measured 2.1e-8 / 4.6e-9, sparse 3.0e-8 / 7.7e-9


# ---- planted rounding-edge inputs: the CPU guards of test_gpu_bext_planted.py
# and test_gpu_decode_planted.py (the reference checked on exactly the inputs
# the GPU parity tests plant) ----

PLANT_N = 1 << 10  # a coefficient's basis extension does not depend on the degree
PLANT_CASES = [(name, lvl) for name, p in PLANT_CHAINS.items() for lvl in p["levels"]]


def _plant_oracle(oracle_mod, name):
    """the chain's primes (made for its own degree) under an oracle of degree PLANT_N"""
    p = PLANT_CHAINS[name]
    mods = oracle_mod.gen_moduli(p["logn"], p["logq"], p["logp"])
    return oracle_mod.Oracle(PLANT_N.bit_length() - 1, mods, len(p["logq"]), len(p["logp"])), mods


def _bext_restated(s, ts, x, centred):
    """Lattigo's ModUpExact of x [len(s)][n] (sources s, targets ts) in Python
    integers, the quotient in numpy float64: correctly rounded divisions
    accumulated in source order, truncated.  A one-prime centred digit extends
    x - s for x >= s >> 1.  Returns (out [len(ts)][n], quotients [len(s)][n])."""
    n = x.shape[1]
    S = 1
    for si in s:
        S *= si
    if centred and len(s) == 1:
        y = [[int(a) for a in x[0]]]
        quo = np.zeros((1, n))
        v = [int(a >= s[0] >> 1) for a in y[0]]
    else:
        y, quo = [], np.zeros((len(s), n))
        for i, si in enumerate(s):
            inv = pow(S // si, -1, si)
            y.append([int(a) * inv % si for a in x[i]])
            quo[i] = np.array(y[i], dtype=np.uint64).astype(np.float64) / np.float64(si)
        vf = np.zeros(n)
        for i in range(len(s)):
            vf = vf + quo[i]
        v = [int(a) for a in vf]
    out = np.zeros((len(ts), n), dtype=np.uint64)
    for k, t in enumerate(ts):
        qh = [S // si % t for si in s]
        out[k] = [(sum(y[i][c] * qh[i] for i in range(len(s))) - v[c] * S) % t for c in range(n)]
    return out, quo


def _quotient_sensitive(quo):
    """per coefficient: does moving any one quotient by one ulp change trunc(sum)?"""
    def tsum(q):
        vf = np.zeros(q.shape[1])
        for row in q:
            vf = vf + row
        return np.trunc(vf)

    base = tsum(quo)
    sens = np.zeros(quo.shape[1], dtype=bool)
    for i in range(quo.shape[0]):
        for to in (-np.inf, np.inf):
            q2 = quo.copy()
            q2[i] = np.nextafter(quo[i], to)
            sens |= tsum(q2) != base
    return sens


@pytest.mark.parametrize("name,level", PLANT_CASES)
def test_planted_modup_matches_restatement(oracle_mod, name, level):
    """plant_digit_values' limbs through orc.modup_digit, digit by digit onto
    every other QP modulus of the level, equal the big-integer / float64
    restatement; the planting is what it says (3/4 of a multi-limb digit's
    coefficients within 2^50 of 0 or S, limbs = X mod q_j); and on at least a
    quarter of those coefficients a one-ulp move of one quotient changes the
    truncated sum (measured 0.45-0.74 on X = delta and X = S - 1 - delta alone,
    0 of 4000 on uniformly random X): the parity tests on these inputs tell a
    correctly rounded quotient from a nearly right one."""
    orc, mods = _plant_oracle(oracle_mod, name)
    K = orc.K
    rng = np.random.default_rng(1000 + level)
    w, X = plant_digit_values(rng, mods, level, K, PLANT_N)
    assert w.shape == (level + 1, PLANT_N) and w.dtype == np.uint64
    for i, limbs in enumerate(digit_limbs(level, K)):
        s = [mods[j] for j in limbs]
        S = int(np.prod([int(v) for v in s], dtype=object))
        for j in limbs:
            assert [int(a) for a in w[j]] == [x % mods[j] for x in X[i]]
        dst = [m for m in orc.qp_mods(level) if m not in limbs]
        got = orc.modup_digit(w[limbs[0]:limbs[-1] + 1], limbs, dst)
        ref, quo = _bext_restated(s, [mods[m] for m in dst], w[limbs[0]:limbs[-1] + 1], True)
        assert np.array_equal(got, ref), (name, level, i)
        if len(limbs) == 1:
            half = s[0] >> 1
            assert {0, 1, half - 1, half, half + 1, s[0] - 1} <= set(X[i])
            continue
        near = sum(1 for x in X[i] if min(x, S - 1 - x) < 1 << 50)
        assert near >= 3 * PLANT_N // 4, (name, level, i, near)
        share = _quotient_sensitive(quo).mean()
        print(f"{name} level {level} digit {i} ({len(limbs)} limbs): quotient-sensitive share {share:.3f}")
        assert share >= 0.25, (name, level, i, share)


def _unit_key_moddown_sources(oracle_mod, name, level):
    """(oracle, planted integers of digit 0, S_0, the ModDown's sources [K][n]):
    the unit Galois key (digit 0, component 0 = 1; all else 0) makes the gadget
    product's accumulator the ModUp of digit 0 of the planted c1; the ModDown's
    sources are the INTT of its P limbs"""
    orc, mods = _plant_oracle(oracle_mod, name)
    L, K = orc.L, orc.K
    w, X = plant_digit_values(np.random.default_rng(2000 + level), mods, level, K, PLANT_N)
    c1 = np.stack([orc.ntt(j, w[j]) for j in range(level + 1)])
    key = np.zeros((orc.dnum, 2, L + K, PLANT_N), dtype=np.uint64)
    key[0, 0] = 1
    u0, u1 = orc.gadget_product_lazy(c1, key, level)
    assert not u1.any()
    xp = np.stack([orc.intt(L + k, u0[level + 1 + k]) for k in range(K)])
    S0 = int(np.prod([mods[j] for j in digit_limbs(level, K)[0]], dtype=object))
    return orc, X[0], S0, xp


def _near_zero_mod_p(orc, xp):
    small = np.ones(xp.shape[1], dtype=bool)
    for k in range(orc.K):
        p = orc.moduli[orc.L + k]
        small &= np.array([min(int(a), p - int(a)) <= 1 << 51 for a in xp[k]])
    return small


def test_planted_unit_key_plants_the_moddown(oracle_mod):
    """SMALL at level 5: the ModDown's sources under the unit key are the
    planted integers again.  Of the coefficients planted within 2^51 of 0 or of
    S_0 (3/4 of all: one in eight is the uniformly random control and one in
    eight sits on a target's edge, neither near 0, so no share of all
    coefficients can reach 7/8), at least 90 % arrive within 2^51 of 0 mod
    both p.  Measured 0.93: 0.99 of X = delta, 0.86 of X = S_0 - 1 - delta (a
    near-S_0 value whose float quotient is the exact floor arrives as X, one
    whose quotient is one high as -(1 + delta))."""
    orc, X0, S0, xp = _unit_key_moddown_sources(oracle_mod, "small", 5)
    planted = np.array([min(x, S0 - x) <= 1 << 51 for x in X0])
    small = _near_zero_mod_p(orc, xp)
    share = (small & planted).sum() / planted.sum()
    print(f"planted {planted.mean():.3f}, of which arrive {share:.3f}; of all {small.mean():.3f}")
    assert planted.mean() >= 0.75
    assert share >= 0.90, share


@pytest.mark.parametrize("name,level", [("small", 5), ("small", 1), ("k8", 16), ("n15", 5)])
def test_planted_moddown_matches_restatement(oracle_mod, name, level):
    """Every chain and level of the planted ModDown tests: on the sources the
    unit key leaves, orc.basis_extend (the ModDown's extension P -> Q) equals
    the big-integer / float64 restatement, and a one-ulp move of one quotient
    changes the truncated sum on at least a quarter of the coefficients (the
    condition of test_planted_modup_matches_restatement: with eight 61-bit
    sources only 0.87 of the planted values arrive near 0 mod p -- their
    float quotient truncates one low more often -- but the sum still sits on
    an integer)."""
    orc, X0, S0, xp = _unit_key_moddown_sources(oracle_mod, name, level)
    L, K, mods = orc.L, orc.K, orc.moduli
    src, dst = [L + k for k in range(K)], list(range(level + 1))
    ref, quo = _bext_restated([mods[m] for m in src], [mods[m] for m in dst], xp, False)
    assert np.array_equal(orc.basis_extend(xp, src, dst), ref)
    share = _quotient_sensitive(quo).mean()
    print(f"{name} level {level}: near 0 mod p {_near_zero_mod_p(orc, xp).mean():.3f}, quotient-sensitive {share:.3f}")
    assert share >= 0.25, share


@pytest.mark.parametrize("name,level,ci", [("small", 0, False), ("small", 1, False), ("small", 3, False),
                                           ("small", 5, False), ("small", 3, True), ("k8", 16, False)])
def test_decode_of_constant_is_the_rounded_integer(oracle_mod, name, level, ci):
    """The NTT of the constant polynomial X is the constant row X mod q_j, and
    every slot of its decoding is float(X centred) / scale exactly: one
    correctly rounded conversion of the exact integer (Lattigo:
    big.Float.SetInt(x).Float64(), then / scale); the special FFT of a lone
    coefficient 0 only adds zeros.  X on the edges of the CRT, the conversion
    and the centring (helpers.decode_edge_values)."""
    p = PLANT_CHAINS[name]
    mods = oracle_mod.gen_moduli(p["logn"] + ci, p["logq"], p["logp"])
    orc = oracle_mod.Oracle(7, mods, len(p["logq"]), len(p["logp"]), ci=ci)
    qs = mods[:level + 1]
    sp, sweep = decode_edge_values(np.random.default_rng(3000 + level), qs)
    xs = sp + sweep
    rows = constant_rows(xs, qs, orc.N)
    for scale in (2.0 ** 40, 3 * 2.0 ** 38):
        for b, x in enumerate(xs):
            got = orc.decode(rows[b], level, scale)
            assert got.shape == (orc.slots,) and np.all(got == float(x) / scale), (x, scale, got[0])


# ---- the encoder's fixed-point rule on planted edges (CPU guards of tests/test_gpu_encode_planted.py) ----
def _planted_encode_oracle(oracle_mod, name, ci):
    p = PLANT_CHAINS[name]
    mods = oracle_mod.gen_moduli(p["logn"] + ci, p["logq"], p["logp"])
    q60 = oracle_mod.gen_moduli(14, [60], [])[0]
    return oracle_mod.Oracle(8, mods, len(p["logq"]), len(p["logp"]), ci=ci), encode_planted_cases(mods, q60)


@pytest.mark.parametrize("name,ci", [("small", False), ("small", True), ("k1", False)])
def test_planted_encode_matches_the_rule(oracle_mod, name, ci):
    """An image whose every slot is c encodes to the constant polynomial
    rule(fl(c * scale)): the special iFFT's sums double, its differences are
    zero, and n c (1/n) is exact.  The oracle's encode against the Python
    restatement of the fixed-point rule (helpers.fixed_point_rule), exact
    integers, on every planted (c, scale) with both signs; chains with a 55-bit
    and a 60-bit first prime, both rings (the rule does not depend on the degree)."""
    orc, cases = _planted_encode_oracle(oracle_mod, name, ci)
    level = 5
    qs, mods = orc.moduli[:level + 1], list(range(level + 1))
    assert len({n for n, _, _ in cases}) == len(cases)
    for scale, imgs in planted_batches(cases).items():
        for nm, c in imgs:
            got = orc.encode(np.full(orc.slots, np.float64(np.float32(c))), scale, mods)
            exp = constant_rows([fixed_point_rule(c, scale)], qs, orc.N)[0]
            assert np.array_equal(got, exp), (nm, c, scale, got[:, 0], exp[:, 0])


def _frac(y):
    from fractions import Fraction
    return Fraction(float(abs(y)))


# wrong rules a planted case must tell from the right one: (y, q) -> residue
def _signed(k, y, q):
    return (-k if y < 0 else k) % q


def _wrong_exact_floor(y, q):  # floor(|y| + 1/2) in exact arithmetic
    from fractions import Fraction
    return _signed(int(_frac(y) + Fraction(1, 2)), y, q)


def _wrong_truncate(y, q):
    return _signed(int(_frac(y)), y, q)


def _wrong_half_even(y, q):
    return _signed(round(_frac(y)), y, q)  # Fraction.__round__: ties to even


def _right(y, q):
    a = abs(float(y))
    return _signed(int(np.float64(a) + np.float64(0.5)) if a < 2.0 ** 64 else int(a), y, q)


def _wrong_negative_zero_is_q(y, q):
    r = _right(y, q)
    return q if y < 0 and r == 0 else r


def _wrong_one_word_ends_at_2_63(y, q):
    """'The big path from 2^63'.  Read literally (a >= 2^63 takes int(a))
    that is the right rule: a + 0.5 == a in float64 from 2^53 on, and
    mant * 2^11 is as exact as mant * 2^12.  What a threshold at 2^63 gets
    wrong is the one-word conversion it is there for, a signed one, which
    saturates at 2^63 - 1 while the exact path still starts at 2^64."""
    a = abs(float(y))
    if 2.0 ** 63 <= a < 2.0 ** 64:
        return _signed(2 ** 63 - 1, y, q)
    return _right(y, q)


def test_planted_encode_cases_have_teeth(oracle_mod):
    """Each plausible wrong fixed-point rule disagrees with the right one on at
    least one planted case (with the chain's residues, as the parity tests
    compare them), and the rule of this test is the rule of helpers.py."""
    orc, cases = _planted_encode_oracle(oracle_mod, "small", False)
    qs = orc.moduli[:6]
    ys = []
    for scale, imgs in planted_batches(cases).items():
        for nm, c in imgs:
            ys.append((nm, fixed_point_y(c, scale)))
            assert [_right(ys[-1][1], q) for q in qs] == [fixed_point_rule(c, scale) % q for q in qs], nm
    for wrong in (_wrong_exact_floor, _wrong_truncate, _wrong_half_even, _wrong_negative_zero_is_q,
                  _wrong_one_word_ends_at_2_63):
        caught = [nm for nm, y in ys if [wrong(y, q) for q in qs] != [_right(y, q) for q in qs]]
        print(wrong.__name__, caught)
        assert caught, wrong.__name__


# ---- decode against the canonical embedding evaluated directly (np.longdouble) ----
@pytest.mark.parametrize("logn,ci", [(13, False), (13, True), (15, False), (15, True)])
def test_decode_matches_canonical_embedding(oracle_mod, logn, ci):
    """Slot j of a decoded plaintext is m(zeta^(5^j)) / scale, zeta the
    primitive 2N-th root (4N-th on the ConjugateInvariant ring): the oracle's
    special FFT against helpers.canonical_slots, a direct sum in extended
    precision, on signed coefficients uniform in +-2^45 at scale 2^40."""
    mods = oracle_mod.gen_moduli(logn + ci, SPLIT_CHAIN["logq"], SPLIT_CHAIN["logp"])
    orc = oracle_mod.Oracle(logn, mods, 3, 1, ci=ci)
    m, rows = embedding_plaintext(orc, 500 + logn)
    js = embedding_slots(orc.slots, np.random.default_rng(logn))
    exp = canonical_slots(m, js, ci) / np.longdouble(2.0 ** 40)
    got = orc.decode(rows, 1, 2.0 ** 40)
    dev = float(np.abs(got[js].astype(np.longdouble) - exp).max())
    print(f"logn {logn} ci {ci}: max |slot| {float(np.abs(exp).max()):.3g}, deviation {dev:.3g}")
    assert float(np.abs(exp).max()) > 100
    assert dev <= EMBED_TOL, dev
