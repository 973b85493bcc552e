"""OrionHipMulRelinSum: sum_i a[i] * b[i] with one relinearisation
(include/orion_hip.h; tensor_sum_kernel, Context::mul_relin_sum).  The
expectation is composed from oracle pieces only -- Oracle.mul_coeffs per
component product, the sums taken mod q in numpy, Oracle.keyswitch of D2 with
the exported relinearisation key, the addition -- and every comparison is bit
for bit.

The chain is logQ = [60, 55, 50, 40, 40, 40], logP = [60, 60] at N = 2^13 (the
prime generator accepts every size asked for): one Q prime in each class of
the accumulating kernel's Barrett reduction (at most 52 bits: one reduction
per launch; at most 60: every 4 pairs; 61, the size of the P primes, does not
occur among Q limbs -- tests/cpu/tensor_sum_check.cpp covers it)."""
import threading

import numpy as np
import pytest

from tests.helpers import SMALL, SchemeCache, rand_ct

pytestmark = pytest.mark.gpu

LOGN, LOGQ, LOGP = 13, [60, 55, 50, 40, 40, 40], [60, 60]
TOP = len(LOGQ) - 1
SEED = 1618
SCALE = 2.0 ** 20  # of an imported operand: a product has 2^40, printed exactly by the error messages
MAXTSUM = 16       # orion_amd/csrc/tensor_sum.h ORION_MAXTSUM (test_tensor_sum_plan.py reads it off the header)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_scheme(relin=True, logq=LOGQ, logp=LOGP, seed=SEED):
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(LOGN, logq, logp, 40, h=192, seed=seed)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    if relin:
        lib.GenerateRelinearizationKey()
    return lib


_cache = SchemeCache()


class Env:
    def __init__(self, oracle_mod):
        self.lib = make_scheme()
        self.mods = self.lib.moduli()
        self.orc = oracle_mod.Oracle(LOGN, self.mods, len(LOGQ), len(LOGP))
        self.rlk = self.lib.export_relin_key()


@pytest.fixture
def env(torch_cuda, oracle_mod):
    def make():
        e = Env(oracle_mod)
        return e.lib, e
    return _cache.get(make)[1]


def expected(orc, mods, rlk, a_arrs, b_arrs, level=None):
    """The defined result of the call on the operands a_arrs[i], b_arrs[i]
    (numpy [B_i][2][limbs_i][N]): [B][2][level + 1][N], level = the lowest."""
    n = len(a_arrs)
    if level is None:
        level = min(x.shape[2] for x in list(a_arrs) + list(b_arrs)) - 1
    B = max(x.shape[0] for x in list(a_arrs) + list(b_arrs))
    ml = list(range(level + 1))
    q = np.array([mods[j] for j in ml], dtype=np.uint64)[:, None]
    N = a_arrs[0].shape[-1]
    out = np.zeros((B, 2, level + 1, N), dtype=np.uint64)
    memo = {}

    def prod(x, ix, cx, y, iy, cy):
        key = (id(x), ix, cx, id(y), iy, cy)
        if key not in memo:
            memo[key] = orc.mul_coeffs(x[ix, cx, :level + 1], y[iy, cy, :level + 1], ml)
        return memo[key]

    for img in range(B):
        D = [np.zeros((level + 1, N), dtype=np.uint64) for _ in range(3)]
        for i in range(n):
            a, b = a_arrs[i], b_arrs[i]
            ia, ib = (img if a.shape[0] > 1 else 0), (img if b.shape[0] > 1 else 0)
            # residues are below 2^61: a sum of two fits a uint64
            D[0] = (D[0] + prod(a, ia, 0, b, ib, 0)) % q
            D[1] = (D[1] + prod(a, ia, 0, b, ib, 1)) % q
            D[1] = (D[1] + prod(a, ia, 1, b, ib, 0)) % q
            D[2] = (D[2] + prod(a, ia, 1, b, ib, 1)) % q
        k0, k1 = orc.keyswitch(D[2], rlk, level)
        out[img, 0] = (D[0] + k0) % q
        out[img, 1] = (D[1] + k1) % q
    return out


def delete(lib, handles):
    for h in set(handles):
        lib.DeleteCiphertext(h)


def run_case(env, arrs, pairs, level=None, scale=SCALE):
    """imports arrs, sums the pairs [(ia, ib)] (indices into arrs), compares
    with the expectation; returns the exported result"""
    lib = env.lib
    hs = [lib.import_ciphertext(x, scale) for x in arrs]
    out = lib.mul_relin_sum([hs[i] for i, _ in pairs], [hs[j] for _, j in pairs])
    exp = expected(env.orc, env.mods, env.rlk, [arrs[i] for i, _ in pairs], [arrs[j] for _, j in pairs], level)
    assert lib.GetCiphertextLevel(out) == exp.shape[2] - 1 and lib.GetCiphertextBatch(out) == exp.shape[0]
    assert lib.GetCiphertextScaleF(out) == scale * scale
    got = lib.export_ciphertext(out)
    assert np.array_equal(got, exp)
    delete(lib, hs + [out])
    return got


def distinct_pairs(n, m):
    """n ordered pairs over m operands, no pair twice, squares among them"""
    allp = [(i, (i + d) % m) for d in range(m) for i in range(m)]
    assert n <= len(allp)
    return allp[:n] if n > 3 else [(0, 1), (2, 0), (1, 2)][:n]


# ---- 1. pair counts on either side of the launch size ------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 16, 17, 33])
def test_sum_matches_the_composed_oracle(env, n):
    rng = np.random.default_rng(10 + n)
    arrs = [rand_ct(rng, env.mods, TOP, env.lib.N, B=2) for _ in range(6)]
    pairs = distinct_pairs(n, 6)
    got = run_case(env, arrs, pairs)
    if n == 1:
        lib = env.lib
        ha, hb = (lib.import_ciphertext(arrs[i], SCALE) for i in pairs[0])
        one = lib.MulRelinCiphertextNew(ha, hb)
        assert np.array_equal(lib.export_ciphertext(one), got)
        delete(lib, [ha, hb, one])


# ---- 2. the accumulator bound on the device -------------------------------------------------
@pytest.mark.parametrize("n", [4, 8, 16, 17])
def test_planted_maxima(env, n):
    """every residue of every operand is q_j - 1: each of the 4n products is
    (q - 1)^2, the largest the unreduced sums can hold between reductions"""
    top = np.zeros((2, 2, TOP + 1, env.lib.N), dtype=np.uint64)
    for j in range(TOP + 1):
        top[:, :, j, :] = env.mods[j] - 1
    arrs = [top, top.copy()]
    got = run_case(env, arrs, [(0, 1)] * n)  # two handles: no pair is a square
    assert np.array_equal(got, run_case(env, arrs, [(0, 0)] * n))  # the same values as squares


# ---- 3. squares and repeats -------------------------------------------------------------------
def test_squares_and_repeated_handles(env):
    rng = np.random.default_rng(30)
    x, y = (rand_ct(rng, env.mods, TOP, env.lib.N, B=2) for _ in range(2))
    run_case(env, [x, y], [(0, 0), (0, 1), (1, 1), (1, 0)])
    run_case(env, [x], [(0, 0)] * 16)


# ---- 4. mixed levels ---------------------------------------------------------------------------
def test_mixed_levels_and_level_zero(env):
    rng = np.random.default_rng(40)
    arrs = [rand_ct(rng, env.mods, TOP, env.lib.N, B=2) for _ in range(3)]
    low = rand_ct(rng, env.mods, 3, env.lib.N, B=2)
    got = run_case(env, arrs + [low], [(0, 1), (2, 3), (1, 2)])
    assert got.shape[2] == 4
    zero = [rand_ct(rng, env.mods, 0, env.lib.N, B=2) for _ in range(3)]
    got = run_case(env, zero, [(0, 1), (1, 2), (2, 2)])
    assert got.shape[2] == 1


# ---- 5. broadcast and the widest grid ---------------------------------------------------------
def test_broadcast_and_batch_64(env):
    rng = np.random.default_rng(50)
    a = [rand_ct(rng, env.mods, 2, env.lib.N, B=1) for _ in range(2)]
    b = [rand_ct(rng, env.mods, 2, env.lib.N, B=3) for _ in range(2)]
    got = run_case(env, a + b, [(0, 2), (1, 3), (0, 3)])
    assert got.shape[0] == 3
    wide = [rand_ct(rng, env.mods, 1, env.lib.N, B=64) for _ in range(3)]
    got = run_case(env, wide, [(0, 1), (2, 2)])
    assert got.shape[:3] == (64, 2, 2)


# ---- 6. the rescale that follows ---------------------------------------------------------------
def test_rescale_after_the_call(torch_cuda, oracle_mod, monkeypatch):
    """RescaleNew as the next call: Oracle.rescale of the composed expectation,
    with the library's deferral on (one division by P q_level) and off"""
    level, n = TOP, 3
    rng = np.random.default_rng(60)
    arrs = None
    res = {}
    for defer in (True, False):
        monkeypatch.setenv("ORION_DEFER", "1" if defer else "0")
        lib = make_scheme()
        try:
            mods = lib.moduli()
            if arrs is None:
                arrs = [rand_ct(rng, mods, level, lib.N, B=8) for _ in range(3)]
            hs = [lib.import_ciphertext(x, SCALE) for x in arrs]
            lib.RescaleNew(lib.mul_relin_sum(hs, hs[1:] + hs[:1]))  # (tables: first use)
            lib.OrionHipProfileReset()
            lib.OrionHipProfile(1)
            s = lib.mul_relin_sum(hs, hs[1:] + hs[:1])
            y = lib.RescaleNew(s)
            lib.OrionHipProfile(0)
            prof = {k: v["launches"] for k, v in lib.profile_read().items()}
            assert lib.GetCiphertextLevel(y) == level - 1
            got = lib.export_ciphertext(y)
            orc = oracle_mod.Oracle(LOGN, mods, len(LOGQ), len(LOGP))
            exp = expected(orc, mods, lib.export_relin_key(), arrs, arrs[1:] + arrs[:1])
            for b in range(8):
                assert np.array_equal(got[b], orc.rescale(exp[b], level)), (defer, b)
            res[defer] = (got, prof)
        finally:
            lib.DeleteScheme()
    assert np.array_equal(res[True][0], res[False][0])
    # (the merged division: one forward and one inverse NTT launch fewer than op by op)
    assert res[True][1]["ntt_fwd"] == res[False][1]["ntt_fwd"] - 1, res
    assert res[True][1]["ntt_inv"] == res[False][1]["ntt_inv"] - 1, res
    assert res[True][1]["tensor"] == res[False][1]["tensor"] == 1


# ---- 7. launch counts ----------------------------------------------------------------------------
def profiled(lib, fn):
    lib.OrionHipProfileReset()
    lib.OrionHipProfile(1)
    r = fn()
    lib.OrionHipProfile(0)
    p = lib.profile_read()
    return r, {k: p[k]["launches"] for k in p}


@pytest.mark.parametrize("n", [2, 17])
def test_one_key_switch_whatever_n(env, n):
    """the fused call launches ceil(n / 16) tensor kernels and, in every other
    category, what ONE MulRelinCiphertextNew launches (a loop launches n times that)"""
    lib = env.lib
    rng = np.random.default_rng(70 + n)
    arrs = [rand_ct(rng, env.mods, TOP, lib.N, B=2) for _ in range(2)]
    ha, hb = (lib.import_ciphertext(x, SCALE) for x in arrs)
    made = []

    def single():
        made.append(lib.MulRelinCiphertextNew(ha, hb))
        made.append(lib.RescaleNew(made[-1]))

    def fused():
        made.append(lib.mul_relin_sum([ha] * n, [hb] * n))
        made.append(lib.RescaleNew(made[-1]))

    single(), fused()  # (tables: first use)
    _, A = profiled(lib, single)
    _, F = profiled(lib, fused)
    assert A["tensor"] == 1 and A["ks_mac"] >= 1
    assert F["tensor"] == -(-n // MAXTSUM), (F, A)
    for k in A:
        if k != "tensor":
            assert F[k] == A[k], (k, F, A)
    delete(lib, [ha, hb] + made)


# ---- 8. graph capture ---------------------------------------------------------------------------
def test_captured_call_replays_to_the_same_bits(env):
    lib = env.lib
    rng = np.random.default_rng(80)
    arrs = [rand_ct(rng, env.mods, TOP, lib.N, B=2) for _ in range(3)]
    hs = [lib.import_ciphertext(x, SCALE) for x in arrs]
    a, b = [hs[0], hs[1], hs[2]], [hs[1], hs[2], hs[2]]
    warm = lib.mul_relin_sum(a, b)
    eager = lib.export_ciphertext(warm)
    assert np.array_equal(eager, expected(env.orc, env.mods, env.rlk, [arrs[0], arrs[1], arrs[2]],
                                          [arrs[1], arrs[2], arrs[2]]))
    lib.OrionHipGraphBegin()
    try:
        out = lib.mul_relin_sum(a, b)
    finally:
        gid = lib.OrionHipGraphEnd()
    for _ in range(2):
        assert lib.OrionHipGraphLaunch(gid) == 0
        lib.OrionHipSynchronize()
        assert np.array_equal(lib.export_ciphertext(out), eager)
    lib.OrionHipGraphDestroy(gid)
    delete(lib, hs + [warm, out])


# ---- 9. pipelines -------------------------------------------------------------------------------
def test_pipeline_thread_sums_the_schemes_operands(env):
    """a thread bound to a pipeline context (OrionHipPeerCreate /
    OrionHipPeerSelect) sums operands the scheme's context owns: the bits of
    the same call on the scheme's context; the operands are deleted afterwards"""
    lib = env.lib
    rng = np.random.default_rng(90)
    arrs = [rand_ct(rng, env.mods, TOP, lib.N, B=2) for _ in range(3)]
    hs = [lib.import_ciphertext(x, SCALE) for x in arrs]
    a, b = [hs[0], hs[1], hs[0]], [hs[1], hs[2], hs[0]]
    mine = lib.mul_relin_sum(a, b)
    exp = lib.export_ciphertext(mine)
    peer = lib.OrionHipPeerCreate()
    assert peer >= 1
    res = {}

    def work():
        try:
            assert lib.OrionHipPeerSelect(peer) == 0
            out = lib.mul_relin_sum(a, b)
            res["handle"] = out
            res["bits"] = lib.export_ciphertext(out)
            lib.DeleteCiphertext(out)
        except BaseException as e:  # reported below
            res["error"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "error" not in res, res["error"]
    assert res["handle"] >> 20 == peer
    assert np.array_equal(res["bits"], exp)
    delete(lib, hs + [mine])
    assert np.array_equal(exp, expected(env.orc, env.mods, env.rlk, [arrs[0], arrs[1], arrs[0]],
                                        [arrs[1], arrs[2], arrs[0]]))


# ---- 10. decrypts -------------------------------------------------------------------------------
def test_decrypted_dot_product_is_no_worse_than_the_loop(env):
    """4 pairs of encrypted real vectors at scale 2^40: the fused sum and the
    loop of MulRelinCiphertextNew / AddCiphertext, decrypted and decoded,
    against the float64 dot product.  The loop is the existing behaviour and the
    fused path rounds less (one ModDown, not four); the factor 2 only absorbs
    the sampling spread of two noise maxima."""
    lib = env.lib
    rng = np.random.default_rng(100)
    slots = lib.N // 2
    xs = rng.uniform(-1, 1, (4, 1, slots)).astype(np.float32)
    ys = rng.uniform(-1, 1, (4, 1, slots)).astype(np.float32)
    ref = np.sum(xs.astype(np.float64) * ys.astype(np.float64), axis=0)
    cx = [lib.Encrypt(lib.encode_batch(x, TOP, 1 << 40)) for x in xs]
    cy = [lib.Encrypt(lib.encode_batch(y, TOP, 1 << 40)) for y in ys]
    fused = lib.mul_relin_sum(cx, cy)
    loop = lib.MulRelinCiphertextNew(cx[0], cy[0])
    tmp = []
    for i in range(1, 4):
        tmp.append(lib.MulRelinCiphertextNew(cx[i], cy[i]))
        lib.AddCiphertext(loop, tmp[-1])
    err_f = float(np.abs(lib.decode_f64(lib.Decrypt(fused)) - ref).max())
    err_l = float(np.abs(lib.decode_f64(lib.Decrypt(loop)) - ref).max())
    # the loop itself decrypts to the dot product: fresh-encryption noise of about 2^14 under a scale
    # of 2^40, over 4 products of values below 1, is about 2^-24 = 6e-8
    assert err_l < 1e-6, err_l
    assert err_f <= 2 * err_l, f"fused max |error| {err_f:.3e}, loop max |error| {err_l:.3e}"
    delete(lib, cx + cy + [fused, loop] + tmp)


# ---- 11. errors ---------------------------------------------------------------------------------
def test_errors_allocate_nothing(env):
    from orion_amd.backend import c_int
    lib = env.lib
    rng = np.random.default_rng(110)
    x = rand_ct(rng, env.mods, 2, lib.N, B=2)
    a, b, c = (lib.import_ciphertext(x, SCALE) for _ in range(3))
    three = lib.import_ciphertext(np.concatenate([x, x[:1]]), SCALE)
    scaled = lib.import_ciphertext(x, SCALE)
    lib.SetCiphertextScale(scaled, 2 ** 21)
    live = sorted(lib.GetLiveCiphertexts())
    unknown = max(live) + 1000

    def refused(match, fn, *args):
        with pytest.raises(RuntimeError, match=match):
            fn(*args)
        assert sorted(lib.GetLiveCiphertexts()) == live, match

    two = (c_int * 2)(a, b)
    assert lib.lib.OrionHipMulRelinSum(None, two, 2) == -1 and b"null" in lib.lib.OrionHipLastError()
    assert lib.lib.OrionHipMulRelinSum(two, None, 2) == -1 and b"null" in lib.lib.OrionHipLastError()
    assert lib.lib.OrionHipMulRelinSum(two, two, 0) == -1 and b"at least one pair" in lib.lib.OrionHipLastError()
    assert lib.lib.OrionHipMulRelinSum(two, two, -3) == -1 and b"cannot sum -3" in lib.lib.OrionHipLastError()
    assert sorted(lib.GetLiveCiphertexts()) == live
    refused(f"handle not found: {unknown}", lib.mul_relin_sum, [a, unknown], [b, c])
    refused(f"handle not found: {unknown}", lib.mul_relin_sum, [a, b], [b, unknown])
    refused(rf"{a} \(batch 2\) and {three} \(batch 3\): the batches differ", lib.mul_relin_sum, [a, b], [b, three])
    refused(rf"pair 1 \({c} x {scaled}\) has scale 2199023255552, pair 0 \({a} x {b}\) has scale 1099511627776",
            lib.mul_relin_sum, [a, c], [b, scaled])
    # the same scales go through; equal products of unequal factors too
    half = lib.import_ciphertext(x, SCALE)
    lib.SetCiphertextScale(half, 2 ** 19)
    ok = lib.mul_relin_sum([a, half], [b, scaled])
    assert lib.GetCiphertextScaleF(ok) == 2.0 ** 40
    delete(lib, [a, b, c, three, scaled, half, ok])


def test_missing_relinearisation_key(torch_cuda):
    lib = make_scheme(relin=False, logq=SMALL["logq"], logp=SMALL["logp"])
    try:
        x = rand_ct(np.random.default_rng(111), lib.moduli(), 2, lib.N)
        a, b = (lib.import_ciphertext(x, SCALE) for _ in range(2))
        live = sorted(lib.GetLiveCiphertexts())
        with pytest.raises(RuntimeError, match="relinearization key not generated"):
            lib.mul_relin_sum([a], [b])
        assert sorted(lib.GetLiveCiphertexts()) == live
    finally:
        lib.DeleteScheme()


def test_poisoned_source_is_refused(torch_cuda):
    """an operand whose deferred rotate-and-add failed (an allocation past the
    pool cap, the recipe of test_deferred_rotation_failure_poisons): the call
    returns the poison and allocates nothing"""
    lib = make_scheme(logq=SMALL["logq"], logp=SMALL["logp"], seed=112)
    try:
        lib.AddRotationKey(1)
        rng = np.random.default_rng(112)
        x, y = (lib.import_ciphertext(rand_ct(rng, lib.moduli(), 5, lib.N, B=2), SCALE) for _ in range(2))
        r = lib.RotateNew(x, 1)
        assert lib.AddCiphertext(x, r) == x
        st = lib.pool_stats()
        lib.pool_cap(st["held_bytes"] - st["cached_bytes"])  # nothing new fits
        try:
            with pytest.raises(RuntimeError, match="device memory exhausted"):
                lib.DeleteCiphertext(r)
        finally:
            lib.pool_cap(0)
        live = sorted(lib.GetLiveCiphertexts())
        assert r not in live and x in live
        with pytest.raises(RuntimeError, match="deferred rotation by 1 failed"):
            lib.mul_relin_sum([y, y], [y, x])
        assert sorted(lib.GetLiveCiphertexts()) == live
        out = lib.mul_relin_sum([y, y], [y, y])  # with sound operands the same call goes through
        assert lib.GetCiphertextLevel(out) == 5
    finally:
        lib.DeleteScheme()
