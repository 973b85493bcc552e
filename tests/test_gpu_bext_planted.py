"""The basis extension on its rounding edges.  bext_prep (csrc/common.h) forms
Lattigo's float64 quotient v = trunc(sum_i float64(y_i) / float64(s_i)) with a
Markstein division; the oracle divides.  The two give different ciphertext
words only where a one-ulp difference moves the sum across an integer, which
uniformly random residues never do and integers just above 0 or just below
S = prod s_i do on about half the coefficients (tests/test_oracle.py,
test_planted_modup_matches_restatement, guards that share on these inputs).
helpers.plant_digit_values makes such gadget digits -- and digits that land a
target's reduction on 0, 1, t - 1 and t / 2 -- and the tests bring them to
every kernel that extends a basis through the unchanged C-ABI: the ModUp by
decomposing a planted polynomial, the ModDown through a Galois key whose only
non-zero entry is 1 (digit 0, component 0), so that the accumulator is the
ModUp of digit 0.  Every comparison is bit for bit against the CPU oracle, on
images 0 and B - 1 (the other images are copies of those two)."""
import numpy as np
import pytest

from tests.helpers import PLANT_CHAINS, SchemeCache, load_unit_galois_key, mform, plant_digit_values, qp_blob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


SEED = 1618
ROT_REAL, ROT_UNIT = 3, 7  # rotation steps: with the scheme's own key, with the unit key
_caches = {name: SchemeCache() for name in PLANT_CHAINS}


def make_scheme(oracle_mod, name):
    from orion_amd.backend import HipLibrary
    p = PLANT_CHAINS[name]
    lib = HipLibrary().new_scheme(p["logn"], p["logq"], p["logp"], 40, h=192, seed=SEED)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    lib.GenerateRelinearizationKey()
    return lib, oracle_mod.Oracle(p["logn"], lib.moduli(), len(p["logq"]), len(p["logp"]))


def cached_scheme(oracle_mod, name):
    """a scheme per chain shared by the N = 2^13 tests (default environment)"""
    return _caches[name].get(lambda: make_scheme(oracle_mod, name))


def two_images(B, first, last):
    """[B][...]: image 0 = first, image B - 1 = last, the others copies of the two"""
    out = np.empty((B,) + first.shape, dtype=np.uint64)
    out[0::2] = first
    out[1::2] = last
    out[B - 1] = last
    return out


def planted_poly(rng, orc, level):
    """one planted polynomial [level+1][N] in the NTT domain (the GPU's INTT
    returns the planted limbs exactly: the round trip is tested exact)"""
    w, _ = plant_digit_values(rng, orc.moduli, level, orc.K, orc.N)
    return np.stack([orc.ntt(j, w[j]) for j in range(level + 1)])


def rand_poly(rng, orc, level):
    return np.stack([rng.integers(0, orc.moduli[j], orc.N, dtype=np.uint64) for j in range(level + 1)])


def planted_cts(rng, orc, level, B):
    """[B][2][level+1][N]: c0 random, c1 planted"""
    imgs = [np.stack([rand_poly(rng, orc, level), planted_poly(rng, orc, level)]) for _ in range(2)]
    return two_images(B, imgs[0], imgs[1] if B > 1 else imgs[0])


def ones_cts(rng, orc, level, B):
    """[B][2][level+1][N]: c0 random, c1 the NTT of the constant 1 (an all-ones
    row), so that (a0, a1) x (b0, 1) has d2 = a1: relinearisation decomposes a1"""
    imgs = [np.stack([rand_poly(rng, orc, level), np.ones((level + 1, orc.N), dtype=np.uint64)]) for _ in range(2)]
    return two_images(B, imgs[0], imgs[1])


def profiled(lib, fn):
    lib.OrionHipProfileReset()
    lib.OrionHipProfile(1)
    r = fn()
    lib.OrionHipProfile(0)
    p = lib.profile_read()
    return r, {k: p[k]["launches"] for k in p}


def check_modup(lib, orc, level, B, rng):
    """RotateNew and MulRelinCiphertextNew(a, (random, 1)) decompose the planted
    c1 / a1 with the scheme's own keys; each is read back, rescaled and read
    again, and the product is also rescaled unread (the merged ModDown +
    rescale where the deferral takes it).  Returns the launch counts of the
    rotation and the product."""
    x = planted_cts(rng, orc, level, B)
    y = ones_cts(rng, orc, level, B)
    g = int(lib.GaloisElement(ROT_REAL))
    ca, cb = lib.import_ciphertext(x, 2.0 ** 40), lib.import_ciphertext(y, 2.0 ** 40)

    def run():  # (the export runs a product's pending ModDown on its own)
        cr, cm = lib.RotateNew(ca, ROT_REAL), lib.MulRelinCiphertextNew(ca, cb)
        return cr, cm, lib.export_ciphertext(cr), lib.export_ciphertext(cm)

    for h in run()[:2]:  # (key, tables: first use)
        lib.DeleteCiphertext(h)
    (cr, cm, got_r, got_m), prof = profiled(lib, run)
    cm2 = lib.MulRelinCiphertextNew(ca, cb)
    for h in (cr, cm, cm2):
        assert lib.Rescale(h) == h
    got_rs, got_ms, got_ms2 = (lib.export_ciphertext(h) for h in (cr, cm, cm2))
    gk, rlk = lib.export_galois_key(g), lib.export_relin_key()
    for b in sorted({0, B - 1}):
        ref = orc.rotate(x[b], g, gk, level)
        assert np.array_equal(got_r[b], ref), ("rotate", b)
        assert np.array_equal(got_rs[b], orc.rescale(ref, level)), ("rotate, rescale", b)
        ref = orc.mul_relin(x[b], y[b], rlk, level)
        assert np.array_equal(got_m[b], ref), ("mul_relin", b)
        ref = orc.rescale(ref, level)
        assert np.array_equal(got_ms[b], ref), ("mul_relin, rescale", b)
        assert np.array_equal(got_ms2[b], ref), ("mul_relin -> rescale", b)
    for h in (ca, cb, cr, cm, cm2):
        lib.DeleteCiphertext(h)
    return prof


# (chain, level, B): B = 1 has nc B (level + 1) < 256 limb-transforms, B as given
# otherwise is the least multiple of 8 with nc B (level + 1) >= 256 (nc = 1)
MODUP_CASES = [("small", 5, 1), ("small", 5, 48), ("k4", 7, 1), ("k4", 7, 32), ("k8", 16, 1), ("k8", 16, 16),
               ("k8", 10, 1), ("k8", 10, 24), ("k8", 8, 1), ("k8", 8, 32), ("k1", 5, 1), ("k1", 5, 48)]


@pytest.mark.parametrize("name,level,B", MODUP_CASES)
def test_modup_planted(torch_cuda, oracle_mod, name, level, B):
    """ModUp of planted digits with real keys at N = 2^13 (no NTT prologue at
    this degree: bext_in_prologue needs the two-pass kernels).  decompose() takes
    modup_all_kernel<K'> for B = 1 (nc B (level + 1) < ORION_MODUP_MERGE = 256:
    every digit in one launch) and the per-digit basis_ext_kernel<ns'> for the
    larger B; K', ns' = 2, 4 or 8 by the chain's K and the digit's limbs.
    small: K = 2, lazy targets.  k4: 4-limb digits.  k8: digits of 8, 3 and 1
    limbs at levels 16, 10, 8 (the last centred), 30-bit sources onto 30-bit
    (NARROW) and 60/61-bit (WT) targets, the 60-bit q_0's digit onto 30-bit
    (NT) and 61-bit (LAZY) ones.  k1: K = 1, every digit centred (no float
    quotient: the edges are x = s >> 1 and its neighbours, 0 and s - 1).  The
    rotation's ModDown is moddown()'s separate basis_ext_kernel; the product
    rescaled unread runs basis_ext_rescale_kernel (merged_rescale: level >=
    1 and no fused latency path)."""
    lib, orc = cached_scheme(oracle_mod, name)
    prof = check_modup(lib, orc, level, B, np.random.default_rng(100 * level + B))
    assert prof["basis_ext"] > 0 and prof.get("ntt_bext", 0) == 0, prof


@pytest.mark.parametrize("env,B,fused", [({}, 2, True), ({"ORION_BEXT_FUSE_BELOW": "1024"}, 12, True),
                                         ({"ORION_BEXT_FUSE": "0"}, 2, False)])
def test_modup_planted_ntt_prologue(torch_cuda, oracle_mod, monkeypatch, env, B, fused):
    """The NTT_PRO_BEXT prologues at N = 2^15 (the chain of
    test_runtime_switch_parity, level 5, K = 2).  Default environment, B = 2:
    decompose() forms every digit's extension in the prologue of one forward
    NTT of 36 limb-transforms on the latency kernels (ntt2s.hip, after the
    INTT's rows pass: intt_then_fwd), and the ModDown's 24 likewise.
    ORION_BEXT_FUSE_BELOW=1024, B = 12: 216 limb-transforms, a partial round
    of the 256 CUs, so the two-pass kernels of ntt2.hip with the prologue.
    ORION_BEXT_FUSE=0, B = 2: modup_all_kernel<2> and basis_ext_kernel<2> as
    their own launches at this degree."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib, orc = make_scheme(oracle_mod, "n15")
    prof = check_modup(lib, orc, 5, B, np.random.default_rng(150 + B))
    lib.DeleteScheme()
    if fused:
        assert prof["ntt_bext"] > 0, prof
    else:
        assert prof["basis_ext"] > 0 and prof.get("ntt_bext", 0) == 0, prof


def check_moddown(lib, orc, level, B, rng):
    x = planted_cts(rng, orc, level, B)
    g = int(lib.GaloisElement(ROT_UNIT))
    unit = load_unit_galois_key(lib, orc, g)
    ct = lib.import_ciphertext(x, 2.0 ** 40)

    def run():  # (a rotation runs when its result is read)
        cr = lib.RotateNew(ct, ROT_UNIT)
        return cr, lib.export_ciphertext(cr)

    lib.DeleteCiphertext(run()[0])  # (tables: first use)
    (cr, got), prof = profiled(lib, run)
    assert np.array_equal(lib.export_galois_key(g), unit)  # still the loaded key
    for b in sorted({0, B - 1}):
        assert np.array_equal(got[b], orc.rotate(x[b], g, unit, level)), b
    lib.DeleteCiphertext(cr)
    lib.DeleteCiphertext(ct)
    return prof


@pytest.mark.parametrize("name,level,B", [("small", 5, 1), ("small", 5, 48), ("k8", 16, 2)])
def test_moddown_planted(torch_cuda, oracle_mod, name, level, B):
    """ModDown of planted sources at N = 2^13: under the unit Galois key the
    accumulator's P limbs hold +-delta (test_planted_unit_key_plants_the_moddown
    and test_planted_moddown_matches_restatement, tests/test_oracle.py), which
    moddown() extends with its separate basis_ext_kernel<2> (small: two 60-bit
    P primes, lazy targets; B = 1 and B = 48) or
    basis_ext_kernel<8> (k8: eight 61-bit sources onto the 30-bit limbs, NT,
    and the 60-bit q_0, LAZY), followed by the NTT with the subtract-and-scale
    epilogue and the automorphism."""
    lib, orc = cached_scheme(oracle_mod, name)
    prof = check_moddown(lib, orc, level, B, np.random.default_rng(300 * level + B))
    assert prof["basis_ext"] > 0 and prof.get("ntt_bext", 0) == 0, prof


def test_moddown_planted_ntt_prologue(torch_cuda, oracle_mod):
    """N = 2^15, B = 2, default environment: moddown() takes the fused latency
    path (bext_in_prologue: 2 x 2 x 6 = 24 limb-transforms), the extension of the
    planted P limbs formed in the prologue of the ntt2s.hip forward NTT whose
    epilogue subtracts, scales and scatters by the automorphism."""
    lib, orc = make_scheme(oracle_mod, "n15")
    prof = check_moddown(lib, orc, 5, 2, np.random.default_rng(315))
    lib.DeleteScheme()
    assert prof["ntt_bext"] > 0 and prof.get("basis_ext", 0) == 0, prof


@pytest.mark.parametrize("level,B", [(5, 1), (5, 4), (1, 1), (1, 4)])
def test_moddown_rescale_planted(torch_cuda, oracle_mod, monkeypatch, level, B):
    """basis_ext_rescale_kernel<2> on planted sources (SMALL, N = 2^13): a
    linear transform with the single diagonal 1, loaded as all-ones QP rows
    (the constant 1), under unit Galois keys, so that the accumulator is the
    rotated ModUp of digit 0 of the planted c1; EvaluateLinearTransform leaves
    its ModDown pending (merged_rescale: level >= 1, K <= 8, no fused
    latency path at this degree) and RescaleNew runs both as one division by
    P q_level, at level 1 onto a single output limb.  Against the oracle's
    lt_bsgs -> rescale with the loaded diagonal and key, and identical with
    ORION_DEFER=0 (the separate basis_ext_kernel, then the plain rescale).
    What this sees: the target reductions, the pivot r = ((x_l - e_l) / P + h)
    mod q_l and the lazy sums on sources of +-delta.  What it cannot: a
    quotient v that is one off moves the ModDown by one, and the rescale
    divides that away (round((x +- 1) / q_l) differs with probability
    1 / q_l), so a wrong rounding of the float quotient shows in
    test_moddown_planted, not here."""
    from orion_amd.backend import HipLibrary
    p = PLANT_CHAINS["small"]
    res = {}
    x = None
    for defer in (False, True):
        monkeypatch.setenv("ORION_DEFER", "1" if defer else "0")
        lib = HipLibrary().new_scheme(p["logn"], p["logq"], p["logp"], 40, h=192, seed=SEED)
        lib.GenerateSecretKey()
        orc = oracle_mod.Oracle(p["logn"], lib.moduli(), len(p["logq"]), len(p["logp"]))
        if x is None:
            x = planted_cts(np.random.default_rng(400 * level + B), orc, level, B)
        lt = lib.GenerateLinearTransform([1], [], level, 2.0, "load")
        gels = [int(g) for g in lib.GetLinearTransformRotationKeys(lt) if g != 1]
        assert gels
        gkeys = {g: load_unit_galois_key(lib, orc, g) for g in gels}
        assert all(lib.GetGaloisKeyLevel(g) == level for g in gels)
        lib.LoadPlaintextDiagonal(qp_blob(orc, level, [mform(1, q) for q in orc.moduli]), lt, 1)
        pts = [lib.export_lt_diagonal(lt, 1, level)]
        assert np.all(pts[0] == 1)
        ct = lib.import_ciphertext(x, 2.0 ** 40)
        lib.export_ciphertext(lib.RescaleNew(lib.EvaluateLinearTransform(lt, ct)))  # (tables, plans: first use)

        def run():
            return lib.RescaleNew(lib.EvaluateLinearTransform(lt, ct))

        y, prof = profiled(lib, run)
        assert lib.GetCiphertextLevel(y) == level - 1
        res[defer] = (lib.export_ciphertext(y), prof)
        if defer:
            N1 = lib.GetLinearTransformN1(lt)
            for b in sorted({0, B - 1}):
                ref = orc.rescale(orc.lt_bsgs(x[b], level, [1], pts, N1, gkeys), level)
                assert np.array_equal(res[True][0][b], ref), b
        lib.DeleteScheme()
    assert np.array_equal(res[True][0], res[False][0])
    pm, pu = res[True][1], res[False][1]
    assert pm["basis_ext"] >= 1 and pm["basis_ext"] == pu["basis_ext"], (pm, pu)
    assert pm["ntt_inv"] == pu["ntt_inv"] - 1 and pm["ntt_fwd"] == pu["ntt_fwd"] - 1, (pm, pu)  # the merged route
