"""OrionHipRotateHoisted and OrionHipRotateSum: n rotations of one ciphertext,
or their sum, from one gadget decomposition (include/orion_hip.h;
ks_mac_hoisted_kernel, Context::rotate_hoisted, Context::rotate_sum).

A hoisted output is RotateNew's bit for bit, so it is compared with
Oracle.rotate under the exported key and with an exported RotateNew.  The sum
has its own definition, composed here from oracle pieces only --
gadget_product_lazy, automorphism_ntt, moddown, the sums taken mod q in numpy.
Every comparison is bit for bit unless it decrypts."""
import os
import re
import threading

import numpy as np
import pytest

from tests.helpers import LAT, SMALL, WIDE, SchemeCache, rand_ct, sum_expected

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 2.0 ** 40


def _define(name):
    with open(os.path.join(ROOT, "orion_amd", "csrc", "hoist.h")) as fh:
        return int(re.search(rf"#define\s+{name}\s+(\d+)", fh.read()).group(1))


MAXHOIST = _define("ORION_MAXHOIST")        # keys per ks_mac_hoisted launch
MAXBETA = _define("ORION_HOIST_MAXBETA")    # digits the kernel holds in registers (test_hoist_plan.py checks the rule)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_scheme(chain=SMALL, seed=2718, keys=True):
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(chain["logn"], chain["logq"], chain["logp"], 40, h=192, seed=seed)
    if keys:
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
    return lib


class Env:
    def __init__(self, oracle_mod, chain):
        self.lib = make_scheme(chain)
        self.mods = self.lib.moduli()
        self.orc = oracle_mod.Oracle(chain["logn"], self.mods, len(chain["logq"]), len(chain["logp"]))
        self.top = len(chain["logq"]) - 1
        P = 1
        for k in range(self.lib.K):
            P *= self.mods[self.lib.L + k]
        self.P = P

    def g(self, amount):
        return int(self.lib.GaloisElement(int(amount)))

    def keys(self, amounts):
        """the exported keys of the amounts' Galois elements (after the call
        that made them: a key made for a lower level is replaced)"""
        return {g: self.lib.export_galois_key(g) for g in {self.g(k) for k in amounts} if g != 1}


_caches = {"small": SchemeCache(), "wide": SchemeCache(), "lat": SchemeCache()}
_chains = {"small": SMALL, "wide": WIDE, "lat": LAT}


def _env(name, oracle_mod):
    def make():
        e = Env(oracle_mod, _chains[name])
        return e.lib, e
    return _caches[name].get(make)[1]


@pytest.fixture
def env(torch_cuda, oracle_mod):
    return _env("small", oracle_mod)


@pytest.fixture
def wide(torch_cuda, oracle_mod):
    return _env("wide", oracle_mod)


@pytest.fixture
def lat(torch_cuda, oracle_mod):
    return _env("lat", oracle_mod)


def delete(lib, handles):
    for h in set(handles):
        lib.DeleteCiphertext(h)


def check_hoisted(env, x, amounts, level, rotate_new=False):
    """imports x [B][2][level+1][N], rotates it by all amounts at once and
    compares every output with Oracle.rotate (and RotateNew, exported)"""
    lib, orc = env.lib, env.orc
    B = x.shape[0]
    ct = lib.import_ciphertext(x, SCALE)
    outs = lib.rotate_hoisted(ct, amounts)
    assert len(outs) == len(amounts) and len(set(outs)) == len(outs) and ct not in outs
    keys = env.keys(amounts)
    memo = {}
    for k, h in zip(amounts, outs):
        g = env.g(k)
        assert lib.GetCiphertextLevel(h) == level and lib.GetCiphertextBatch(h) == B
        assert lib.GetCiphertextScaleF(h) == SCALE
        got = lib.export_ciphertext(h)
        if g == 1:
            assert np.array_equal(got, x), k
            continue
        if g not in memo:
            memo[g] = np.stack([orc.rotate(x[b], g, keys[g], level) for b in range(B)])
        assert np.array_equal(got, memo[g]), (k, level, B)
        if rotate_new:
            r = lib.RotateNew(ct, k)
            assert np.array_equal(lib.export_ciphertext(r), got), k  # (the export runs the deferred rotation)
            lib.DeleteCiphertext(r)
    delete(lib, outs + [ct])


def check_sum(env, x, amounts, level):
    lib = env.lib
    ct = lib.import_ciphertext(x, SCALE)
    h = lib.rotate_sum(ct, amounts)
    assert lib.GetCiphertextLevel(h) == level and lib.GetCiphertextBatch(h) == x.shape[0]
    assert lib.GetCiphertextScaleF(h) == SCALE
    got = lib.export_ciphertext(h)
    ref = sum_expected(env.orc, x, [env.g(k) for k in amounts], env.keys(amounts), level)
    assert np.array_equal(got, ref), (amounts, level, x.shape[0])
    delete(lib, [ct, h])
    return got


# ---- 1. hoisted = the oracle = RotateNew ------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("level", [5, 4, 2, 1, 0])  # beta = 3, 3 (a partial last digit), 2, 1, 1
def test_hoisted_equals_oracle_and_rotate_new(env, level, B):
    rng = np.random.default_rng(100 + 10 * level + B)
    x = rand_ct(rng, env.mods, level, env.lib.N, B=B)
    check_hoisted(env, x, [1, 5, -3, 1000, 5, 0], level, rotate_new=True)


# ---- 2. the edges of the keys-per-launch chunks --------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 33, 64])
def test_chunk_edges(env, n):
    assert MAXHOIST == 16
    rng = np.random.default_rng(200 + n)
    x = rand_ct(rng, env.mods, 2, env.lib.N, B=2)
    check_hoisted(env, x, list(range(1, n + 1)), 2)


# ---- 3. decompositions at, just past and far past the register bound ---------------------------
@pytest.mark.parametrize("B", [1, 2])
def test_wide_decomposition(wide, B):
    assert wide.top + 1 == 10 > MAXBETA  # beta = 10 at the top: past the bound
    rng = np.random.default_rng(300 + B)
    x = rand_ct(rng, wide.mods, wide.top, wide.lib.N, B=B)
    check_hoisted(wide, x, [1, -2, 300], wide.top)
    check_sum(wide, x, [1, -2, 300], wide.top)


@pytest.mark.parametrize("beta", [MAXBETA, MAXBETA + 1])
def test_register_bound(wide, beta):
    level = beta - 1  # K = 1
    rng = np.random.default_rng(310 + beta)
    x = rand_ct(rng, wide.mods, level, wide.lib.N, B=2)
    check_hoisted(wide, x, [1, -2, 300], level)


# ---- 4. the latency routes -------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
def test_latency_routes(lat, B):
    rng = np.random.default_rng(400 + B)
    x = rand_ct(rng, lat.mods, 5, lat.lib.N, B=B)
    check_hoisted(lat, x, [1, 7, -4], 5, rotate_new=True)
    check_sum(lat, x, [0, 1, 7], 5)


# ---- 5. the widest grid ----------------------------------------------------------------------------
def test_batch_64(env):
    rng = np.random.default_rng(500)
    x = rand_ct(rng, env.mods, 1, env.lib.N, B=64)
    check_hoisted(env, x, [3, -1], 1)


# ---- 6. the sum equals its definition --------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("level", [5, 2, 0])
@pytest.mark.parametrize("amounts", [[1, 2, 4], [0, 1, 1, -1], [0], [7], list(range(1, 34))],
                         ids=["1-2-4", "0-1-1-m1", "0", "7", "1to33"])
def test_sum_equals_its_definition(env, amounts, level, B):
    rng = np.random.default_rng(600 + 10 * level + B + len(amounts))
    x = rand_ct(rng, env.mods, level, env.lib.N, B=B)
    check_sum(env, x, amounts, level)


# ---- 7. launch counts ------------------------------------------------------------------------------
NTT_CATS = ("ntt_fwd", "ntt_inv", "ntt_bext", "basis_ext")


def profiled(lib, fn):
    lib.OrionHipProfileReset()
    lib.OrionHipProfile(1)
    r = fn()
    lib.OrionHipProfile(0)
    p = lib.profile_read()
    return r, {k: p[k]["launches"] for k in p}


def test_hoisted_launch_counts(env):
    """one decomposition whatever n: every further output adds one ModDown's
    launches, and the gadget products run ceil(n / 16) launches"""
    lib = env.lib
    level = 5
    assert (level + 1 + lib.K - 1) // lib.K <= MAXBETA
    x = rand_ct(np.random.default_rng(700), env.mods, level, lib.N, B=2)
    ct = lib.import_ciphertext(x, SCALE)
    made = []

    def call(n):
        made.extend(lib.rotate_hoisted(ct, list(range(1, n + 1))))

    call(33)  # (keys and tables: first use)
    H = {n: profiled(lib, lambda n=n: call(n))[1] for n in (1, 2, 3, 16, 17, 33)}
    for n in (3, 16, 17, 33):
        for k in NTT_CATS:
            assert H[n].get(k, 0) - H[1].get(k, 0) == (n - 1) * (H[2].get(k, 0) - H[1].get(k, 0)), (n, k, H)
    ntt = lambda h: h.get("ntt_fwd", 0) + h.get("ntt_inv", 0) + h.get("ntt_bext", 0)
    assert 0 < ntt(H[2]) - ntt(H[1]) < ntt(H[1]), H  # the increment has no decomposition
    for n in H:
        assert H[n]["ks_mac"] == -(-n // MAXHOIST), (n, H)
    delete(lib, made + [ct])


def test_sum_launch_counts(env):
    lib = env.lib
    x = rand_ct(np.random.default_rng(710), env.mods, 5, lib.N, B=2)
    ct = lib.import_ciphertext(x, SCALE)
    made = [lib.rotate_sum(ct, list(range(1, 17)))]  # (keys and tables: first use)
    S = {}
    for n in (1, 4, 16):
        h, S[n] = profiled(lib, lambda n=n: lib.rotate_sum(ct, list(range(1, n + 1))))
        made.append(h)
    for n in (4, 16):
        for k in NTT_CATS:
            assert S[n].get(k, 0) == S[1].get(k, 0), (n, k, S)
    for n in S:
        assert S[n]["lt_giant"] == 1 and S[n].get("ks_mac", 0) == 0, (n, S)
    delete(lib, made + [ct])


# ---- 8. graph capture ------------------------------------------------------------------------------
def test_captured_calls_replay_to_the_same_bits(env):
    lib = env.lib
    x = rand_ct(np.random.default_rng(800), env.mods, 4, lib.N, B=2)
    ct = lib.import_ciphertext(x, SCALE)
    amounts = [1, 0, -6, 40]
    warm = lib.rotate_hoisted(ct, amounts)
    warm_sum = lib.rotate_sum(ct, amounts)
    eager = [lib.export_ciphertext(h) for h in warm]
    eager_sum = lib.export_ciphertext(warm_sum)
    lib.OrionHipGraphBegin()
    try:
        outs = lib.rotate_hoisted(ct, amounts)
        s = lib.rotate_sum(ct, amounts)
    finally:
        gid = lib.OrionHipGraphEnd()
    for _ in range(2):
        assert lib.OrionHipGraphLaunch(gid) == 0
        lib.OrionHipSynchronize()
        for h, e in zip(outs, eager):
            assert np.array_equal(lib.export_ciphertext(h), e)
        assert np.array_equal(lib.export_ciphertext(s), eager_sum)
    lib.OrionHipGraphDestroy(gid)
    delete(lib, warm + outs + [warm_sum, s, ct])


# ---- 9. pipelines ----------------------------------------------------------------------------------
def test_pipeline_thread_rotates_the_schemes_ciphertext(env):
    lib = env.lib
    x = rand_ct(np.random.default_rng(900), env.mods, 3, lib.N, B=2)
    ct = lib.import_ciphertext(x, SCALE)
    amounts = [2, 0, -9]
    mine = lib.rotate_hoisted(ct, amounts)
    mine_sum = lib.rotate_sum(ct, amounts)
    exp = [lib.export_ciphertext(h) for h in mine]
    exp_sum = lib.export_ciphertext(mine_sum)
    peer = lib.OrionHipPeerCreate()
    assert peer >= 1
    res = {}

    def work():
        try:
            assert lib.OrionHipPeerSelect(peer) == 0
            outs = lib.rotate_hoisted(ct, amounts)
            s = lib.rotate_sum(ct, amounts)
            res["handles"] = outs + [s]
            res["bits"] = [lib.export_ciphertext(h) for h in outs]
            res["sum"] = lib.export_ciphertext(s)
            delete(lib, outs + [s])
        except BaseException as e:  # reported below
            res["error"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "error" not in res, res["error"]
    assert all(h >> 20 == peer for h in res["handles"])
    for got, e in zip(res["bits"], exp):
        assert np.array_equal(got, e)
    assert np.array_equal(res["sum"], exp_sum)
    delete(lib, mine + [mine_sum, ct])


# ---- 10. decrypts ----------------------------------------------------------------------------------
def test_decrypts(env):
    """hoisted rotations decode to the rolled vector within
    test_rotate_decrypts's bound; the fused sum of 4 rotations decodes to the
    float64 sum of the rolls no worse than twice the RotateNew / AddCiphertext
    loop on the same ciphertext (the loop is the existing behaviour and rounds
    three times where the sum rounds once; the factor 2 only absorbs the
    sampling spread of two noise maxima)"""
    lib = env.lib
    rng = np.random.default_rng(1000)
    slots = lib.N // 2
    vals = rng.standard_normal((1, slots)).astype(np.float32)
    ct = lib.Encrypt(lib.encode_batch(vals, env.top, 1 << 40))
    amounts = [1, 7, -3, 0]
    outs = lib.rotate_hoisted(ct, amounts)
    for k, h in zip(amounts, outs):
        dec = lib.decode_f64(lib.Decrypt(h))[0]
        assert np.abs(dec - np.roll(vals[0].astype(np.float64), -k)).max() < 1e-3, k
    ks = [0, 1, 2, 3]
    ref = sum(np.roll(vals[0].astype(np.float64), -k) for k in ks)
    fused = lib.rotate_sum(ct, ks)
    loop = lib.CloneCiphertext(ct)
    tmp = []
    for k in ks[1:]:
        tmp.append(lib.RotateNew(ct, k))
        lib.AddCiphertext(loop, tmp[-1])
    err_f = float(np.abs(lib.decode_f64(lib.Decrypt(fused))[0] - ref).max())
    err_l = float(np.abs(lib.decode_f64(lib.Decrypt(loop))[0] - ref).max())
    print(f"rotate_sum max |error| {err_f:.3e}, loop max |error| {err_l:.3e}")
    # the loop itself decrypts to the sum: fresh-encryption and key-switch noise of about 2^16 under a
    # scale of 2^40, over 4 terms, is about 2^-22 = 2.4e-7
    assert err_l < 1e-6, err_l
    assert err_f <= 2 * err_l, f"fused max |error| {err_f:.3e}, loop max |error| {err_l:.3e}"
    delete(lib, outs + tmp + [fused, loop, ct])


# ---- 11. errors ------------------------------------------------------------------------------------
def _out(n=2):
    from orion_amd.backend import c_int
    return (c_int * n)(*([-7] * n))


def test_errors_allocate_nothing(env):
    from orion_amd.backend import c_int
    lib = env.lib
    x = rand_ct(np.random.default_rng(1100), env.mods, 2, lib.N, B=2)
    ct = lib.import_ciphertext(x, SCALE)
    live = sorted(lib.GetLiveCiphertexts())
    unknown = max(live) + 1000
    two = (c_int * 2)(1, 2)
    big = (c_int * 65)(*range(1, 66))
    H, S, err = lib.lib.OrionHipRotateHoisted, lib.lib.OrionHipRotateSum, lib.lib.OrionHipLastError

    def refused(match, id_, amounts, n, with_out=True):
        out = _out(max(n, 2))
        assert H(id_, amounts, n, out if with_out else None) == -1 and match in err(), (match, err())
        assert list(out) == [-7] * len(out)
        if with_out:
            assert S(id_, amounts, n) == -1 and match in err(), (match, err())
        assert sorted(lib.GetLiveCiphertexts()) == live, match

    refused(b"null", ct, None, 2)
    refused(b"null", ct, two, 2, with_out=False)
    refused(b"0 amounts", ct, two, 0)
    refused(b"-3 amounts", ct, two, -3)
    refused(b"65 amounts in one call: 1 to 64", ct, big, 65)  # the number and the limit are named
    refused(f"handle not found: {unknown}".encode(), unknown, two, 2)
    delete(lib, [ct])


def test_poisoned_source_is_refused(torch_cuda):
    """a source whose deferred rotate-and-add failed (an allocation past the
    pool cap, the recipe of test_deferred_rotation_failure_poisons): both calls
    return the poison and allocate nothing"""
    lib = make_scheme(seed=1112)
    try:
        lib.AddRotationKey(1)
        rng = np.random.default_rng(1112)
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
        out = _out()
        from orion_amd.backend import c_int
        two = (c_int * 2)(1, 2)
        assert lib.lib.OrionHipRotateHoisted(x, two, 2, out) == -1
        assert b"deferred rotation by 1 failed" in lib.lib.OrionHipLastError()
        assert list(out) == [-7, -7]
        with pytest.raises(RuntimeError, match="deferred rotation by 1 failed"):
            lib.rotate_sum(x, [1, 2])
        assert sorted(lib.GetLiveCiphertexts()) == live
        outs = lib.rotate_hoisted(y, [1, 2])  # with a sound source the same call goes through
        assert all(lib.GetCiphertextLevel(h) == 5 for h in outs)
    finally:
        lib.DeleteScheme()


def test_missing_key_without_the_secret_key(torch_cuda):
    """a scheme that imported a key bundle without the secret has the key of
    amount 1 and lacks the key of amount 2: Rotate's message, before anything
    is allocated -- no output for the key that exists"""
    torch = torch_cuda
    from orion_amd.backend import c_int
    lib = make_scheme(seed=1120)
    try:
        lib.AddRotationKey(1)
        n = lib.KeyBundleBytes(0)
        buf = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert lib.lib.ExportKeyBundle(buf.data_ptr(), 0) == 0
        lib.OrionHipSynchronize()
        lib.DeleteScheme()
        lib.new_scheme(SMALL["logn"], SMALL["logq"], SMALL["logp"], 40, h=192, seed=1121)
        assert lib.lib.ImportKeyBundle(buf.data_ptr(), n) == 0, lib.lib.OrionHipLastError()
        x = lib.import_ciphertext(rand_ct(np.random.default_rng(1120), lib.moduli(), 5, lib.N, B=2), SCALE)
        live = sorted(lib.GetLiveCiphertexts())
        with pytest.raises(RuntimeError, match="secret key not generated") as rot:
            lib.Rotate(x, 2)
        out = _out()
        assert lib.lib.OrionHipRotateHoisted(x, (c_int * 2)(1, 2), 2, out) == -1
        assert lib.lib.OrionHipLastError().decode() in str(rot.value)  # Rotate's message
        assert list(out) == [-7, -7]
        with pytest.raises(RuntimeError, match="secret key not generated"):
            lib.rotate_sum(x, [1, 2])
        assert sorted(lib.GetLiveCiphertexts()) == live
        outs = lib.rotate_hoisted(x, [1, 0])  # the key that exists serves
        assert len(outs) == 2
    finally:
        lib.DeleteScheme()
