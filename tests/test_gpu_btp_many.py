"""Slot-packed bootstrapping: OrionHipPackMonomials, OrionHipUnpackMonomials,
OrionHipSlotTraceNew and OrionHipBootstrapMany (include/orion_hip.h;
mono_pack_kernel, mono_unpack_kernel, Context::slot_trace, bootstrap_many).

The expectations are composed from oracle pieces only -- Oracle.ntt of the
unit vectors for M_k, Oracle.mul_coeffs, numpy sums mod q, Oracle.rotate with
the exported Galois keys, Oracle.bootstrap of the full-slot circuit -- or from
the library's own public calls, and every parity comparison is bit for bit.

One scheme serves the module: N = 2^13, residual chain [60] + [40] x 5, logP
[60, 60], bootstrapping P [61, 61], h = 192 (the environment of
test_gpu_complex_pack.py), with the full-slot bootstrapper, and a sparse one
(N/16 slots) for the comparisons only."""
import threading

import numpy as np
import pytest

from tests.helpers import SMALL, SchemeCache, bootstrap_keys, bootstrap_oracle, rand_ct
from tests.slot_pack_helpers import mono, pack, unpack

pytestmark = pytest.mark.gpu

LOGN, LOGQ, LOGP, BTP_LOGP = 13, [60] + [40] * 5, [60, 60], [61, 61]
TOP = len(LOGQ) - 1
N = 1 << LOGN
FULL = N // 2
SCALE = 2.0 ** 20  # of an imported operand: printed exactly by the error messages
SEED = 31415


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_scheme(logq=LOGQ, logp=LOGP, seed=SEED, **kw):
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(LOGN, logq, logp, 40, h=192, seed=seed, **kw)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    lib.GenerateRelinearizationKey()
    return lib


_cache = SchemeCache()


def steps(ns):
    """the rotation amounts of the trace over the slots at distance ns"""
    out = []
    while ns < FULL:
        out.append(ns)
        ns *= 2
    return out


class Env:
    def __init__(self, oracle_mod):
        self.oracle_mod = oracle_mod
        lib = self.lib = make_scheme()
        self.mods = lib.moduli()
        self.orc = oracle_mod.Oracle(LOGN, self.mods, len(LOGQ), len(LOGP))
        # one warm call of everything, then the keys: a key made again for a higher level is a new key
        warm = lib.Encrypt(lib.encode_batch(np.zeros((3, FULL), dtype=np.float32), 0, 1 << 40))
        made = [warm]
        for ns in (FULL, N // 16):
            lib.NewBootstrapper(BTP_LOGP, ns)
            made.append(lib.Bootstrap(warm, ns))
        for ns in (N // 16, N // 4, FULL):
            made.append(lib.bootstrap_many(warm, ns))
        for mean in (False, True):
            made.append(lib.slot_trace_new(made[-2], N // 16, mean))
        made.append(lib.pack_monomials(made[-1], 8))
        made.append(lib.unpack_monomials(made[-1], 8, 3))
        delete(lib, made)
        self.gel = {k: int(lib.GaloisElement(k)) for k in steps(N // 16)}
        self.gk = {k: lib.export_galois_key(g) for k, g in self.gel.items()}
        self.boot, self.circ = bootstrap_oracle(oracle_mod, lib, LOGN, 40, FULL, BTP_LOGP)
        self.keys = bootstrap_keys(lib, FULL)

    def q(self, level):
        return np.array(self.mods[:level + 1], dtype=np.uint64)[:, None]

    def over_g(self, x, g):
        """(g^-1 mod q_l) o x in Python integers, x [..][limbs][N]"""
        out = np.empty_like(x)
        for j in range(x.shape[-2]):
            q = self.mods[j]
            out[..., j, :] = (x[..., j, :].astype(object) * pow(g, -1, q) % q).astype(np.uint64)
        return out

    def trace(self, x, ns, mean):
        """OrionHipSlotTraceNew composed: x [B][2][level + 1][N]"""
        lv = x.shape[2] - 1
        t = self.over_g(x, FULL // ns) if mean else x
        for k in steps(ns):
            r = np.stack([self.orc.rotate(t[b], self.gel[k], self.gk[k], lv) for b in range(t.shape[0])])
            t = (t + r) % self.q(lv)  # residues below 2^61: the sum fits
        return t


@pytest.fixture
def env(torch_cuda, oracle_mod):
    def make():
        e = Env(oracle_mod)
        return e.lib, e
    return _cache.get(make)[1]


def delete(lib, handles):
    for h in set(handles):
        lib.DeleteCiphertext(h)


def profiled(lib, fn):
    lib.OrionHipProfileReset()
    lib.OrionHipProfile(1)
    r = fn()
    lib.OrionHipProfile(0)
    return r, lib.profile_read()


def in_use(lib):
    st = lib.pool_stats()
    return st["held_bytes"] - st["cached_bytes"]


def images(ns, B, seed, dense=False):
    """B real images and what Bootstrap(ct, ns) returns for them: slot k = sum_j in[(k mod ns) + ns j].  Sparse
    images are uniform in (-1, 1) on the first ns slots and zero after; dense ones fill every slot with uniform
    values in (-1/g, 1/g), so that the slot sums stay in (-1, 1), the range the circuit is made for"""
    g = FULL // ns
    vals = np.random.default_rng(seed).uniform(-1, 1, (B, FULL)).astype(np.float32)
    if dense:
        vals = (vals / g).astype(np.float32)
    else:
        vals[:, ns:] = 0
    sums = vals.astype(np.float64).reshape(B, g, ns).sum(axis=1)
    return vals, np.tile(sums, (1, g))


def meta(lib, h):
    return lib.GetCiphertextLevel(h), lib.GetCiphertextBatch(h), lib.GetCiphertextScaleF(h)


# ---- 1. pack / unpack ----------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, TOP])
@pytest.mark.parametrize("B,g", [(8, 8), (3, 8), (9, 8), (4, 2), (1, 8), (64, 4)])
def test_pack_and_unpack_match_the_composition(env, B, g, level):
    lib = env.lib
    x = rand_ct(np.random.default_rng(1000 * B + 10 * g + level), env.mods, level, N, B=B)
    h = -(-B // g)
    hx = lib.import_ciphertext(x, SCALE)
    hp = lib.pack_monomials(hx, g)
    assert meta(lib, hp) == (level, h, SCALE)
    ep = pack(env.orc, x, g)
    assert np.array_equal(lib.export_ciphertext(hp), ep)
    hu = lib.unpack_monomials(hp, g, B)
    assert meta(lib, hu) == (level, B, SCALE)
    got = lib.export_ciphertext(hu)
    assert np.array_equal(got, unpack(env.orc, ep, g, B))
    assert np.array_equal(got[:h], ep)  # the images at X^0 are their groups
    delete(lib, [hx, hp, hu])


@pytest.mark.parametrize("kind", ["max", "mixed"])
def test_pack_and_unpack_planted_maxima(env, kind):
    """every residue q - 1 (each product and each partial sum wraps), or 0 and q - 1 mixed, through the 7-step
    running product of g = 8; the expectation in Python integers on the 60-bit limb and on a 40-bit limb"""
    lib = env.lib
    B = g = 8
    x = np.zeros((B, 2, TOP + 1, N), dtype=np.uint64)
    pick = np.random.default_rng(7).integers(0, 2, (B, 2, TOP + 1, N)).astype(bool)
    for j in range(TOP + 1):
        x[:, :, j, :] = env.mods[j] - 1
    if kind == "mixed":
        x[pick] = 0
    hx = lib.import_ciphertext(x, SCALE)
    hp = lib.pack_monomials(hx, g)
    hu = lib.unpack_monomials(hp, g, B)
    gp, gu = lib.export_ciphertext(hp), lib.export_ciphertext(hu)
    for j in (0, TOP):  # 60 bits, 40 bits
        q = env.mods[j]
        m1 = mono(env.orc, 1, j + 1)[j].astype(object)
        mi = mono(env.orc, -1, j + 1)[j].astype(object)
        assert all((m1 * mi % q) == 1)
        for c in range(2):
            acc, f = x[0, c, j].astype(object), 1
            for i in range(1, g):
                f = f * m1 % q
                acc = (acc + f * x[i, c, j].astype(object)) % q
            assert np.array_equal(gp[0, c, j], acc.astype(np.uint64)), (j, c)
            f = 1
            for i in range(g):
                assert np.array_equal(gu[i, c, j], (f * acc % q).astype(np.uint64)), (j, c, i)
                f = f * mi % q
    delete(lib, [hx, hp, hu])


def test_pack_and_unpack_are_one_launch_each_with_the_stated_bytes(env):
    lib = env.lib
    x = rand_ct(np.random.default_rng(12), env.mods, TOP, N, B=9)
    hx = lib.import_ciphertext(x, SCALE)
    hp, P = profiled(lib, lambda: lib.pack_monomials(hx, 8))
    hu, U = profiled(lib, lambda: lib.unpack_monomials(hp, 8, 9))
    # per (comp, limb, group) row its images and one more, per limb the factor row: (2 (9 + 2) + 1) 8 N per limb
    want = (2 * (9 + 2) + 1) * 8 * N * (TOP + 1)
    assert P["mono_pack"]["launches"] == 1 and sum(v["launches"] for v in P.values()) == 1, P
    assert U["mono_unpack"]["launches"] == 1 and sum(v["launches"] for v in U.values()) == 1, U
    assert P["mono_pack"]["bytes"] == U["mono_unpack"]["bytes"] == want
    delete(lib, [hx, hp, hu])


# ---- 2. the slot trace ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, TOP])
@pytest.mark.parametrize("g", [2, 8])
def test_slot_trace_equals_the_rotation_loop_and_the_oracle(env, g, level):
    lib = env.lib
    ns = FULL // g
    x = rand_ct(np.random.default_rng(200 + 10 * g + level), env.mods, level, N, B=2)
    ginv = env.over_g(x, g)
    hx = lib.import_ciphertext(x, SCALE)
    for mean in (False, True):
        got = lib.slot_trace_new(hx, ns, mean)
        assert meta(lib, got) == (level, 2, SCALE)
        bits = lib.export_ciphertext(got)
        assert np.array_equal(bits, env.trace(x, ns, mean)), mean
        # the public loop: t = t + Rotate(t, ns 2^s), on g^-1 o x for the mean
        t = lib.import_ciphertext(ginv if mean else x, SCALE)
        made = [got]
        for k in steps(ns):
            r = lib.RotateNew(t, k)
            s = lib.AddCiphertextNew(t, r)
            made += [t, r]
            t = s
        assert np.array_equal(bits, lib.export_ciphertext(t)), mean
        delete(lib, made + [t])
    delete(lib, [hx])


def test_slot_trace_over_every_slot_is_a_copy(env):
    lib = env.lib
    x = rand_ct(np.random.default_rng(21), env.mods, TOP, N, B=2)
    hx = lib.import_ciphertext(x, SCALE)
    for mean in (False, True):
        c, P = profiled(lib, lambda: lib.slot_trace_new(hx, FULL, mean))
        assert c != hx and meta(lib, c) == (TOP, 2, SCALE)
        assert np.array_equal(lib.export_ciphertext(c), x)
        assert P["ks_mac"]["launches"] == 0 and P["elementwise"]["launches"] == 1, P
        delete(lib, [c])
    delete(lib, [hx])


@pytest.mark.parametrize("g", [2, 8])
def test_slot_trace_decrypts_to_the_slot_sums_and_means(env, g):
    """dense images: slot k of the sum trace is the sum of the g slots k + ns j, of the mean trace their mean.
    Bar: test_bootstrap_parity's 1e-6 for a fresh scale-2^40 encryption per summed term (every rotation adds
    key-switch noise of that order), so g x 1e-6 for the sum and 1e-6 for the mean"""
    lib = env.lib
    ns = FULL // g
    vals = np.random.default_rng(22 + g).uniform(-1, 1, (2, FULL)).astype(np.float32)
    sums = np.tile(vals.astype(np.float64).reshape(2, g, ns).sum(axis=1), (1, g))
    ct = lib.Encrypt(lib.encode_batch(vals, TOP, 1 << 40))
    s, m = lib.slot_trace_new(ct, ns), lib.slot_trace_new(ct, ns, mean=True)
    es = float(np.abs(lib.decode_f64(lib.Decrypt(s)) - sums).max())
    em = float(np.abs(lib.decode_f64(lib.Decrypt(m)) - sums / g).max())
    print("slot trace g = %d max |error|: sum %.3g mean %.3g" % (g, es, em))
    assert es < g * 1e-6 and em < 1e-6, (es, em)
    delete(lib, [ct, s, m])


# ---- 3. OrionHipBootstrapMany --------------------------------------------------------------------
def composition(lib, ct, ns, B):
    """the public calls OrionHipBootstrapMany stands for; returns (result, every handle made)"""
    g = FULL // ns
    x = lib.CloneCiphertext(ct)
    while lib.GetCiphertextLevel(x) > 0:
        lib.ModDropCiphertext(x)
    u = lib.slot_trace_new(x, ns, mean=True)
    p = lib.pack_monomials(u, g)
    r = lib.Bootstrap(p, FULL)
    w = lib.unpack_monomials(r, g, B)
    out = lib.slot_trace_new(w, ns)
    return out, [x, u, p, r, w, out]


@pytest.mark.parametrize("B,g", [(8, 8), (4, 2), (3, 8)])
def test_bootstrap_many_equals_the_public_composition(env, B, g):
    lib = env.lib
    ns = FULL // g
    vals, _ = images(ns, B, 300 + B)
    ct = lib.Encrypt(lib.encode_batch(vals, 2, 1 << 40))  # above level 0: only limb 0 is read
    out = lib.bootstrap_many(ct, ns)
    comp, made = composition(lib, ct, ns, B)
    assert lib.GetCiphertextBatch(made[2]) == -(-B // g)
    assert meta(lib, out) == meta(lib, comp) == (TOP, B, lib.GetCiphertextScaleF(made[3]))
    assert lib.GetCiphertextSlots(out) == lib.GetCiphertextSlots(made[3])
    assert np.array_equal(lib.export_ciphertext(out), lib.export_ciphertext(comp))
    delete(lib, [ct, out] + made)


def test_bootstrap_many_over_every_slot_is_bootstrap(env):
    lib = env.lib
    vals, _ = images(FULL, 2, 31)
    ct = lib.Encrypt(lib.encode_batch(vals, 2, 1 << 40))
    a, b = lib.bootstrap_many(ct, FULL), lib.Bootstrap(ct, FULL)
    assert meta(lib, a) == meta(lib, b)
    assert np.array_equal(lib.export_ciphertext(a), lib.export_ciphertext(b))
    delete(lib, [ct, a, b])


def test_bootstrap_many_matches_the_oracle(env):
    """B = 3, g = 8: the composed mean trace and pack at level 0, Oracle.bootstrap of the full-slot circuit on
    the one packed ciphertext, the composed unpack and sum trace at the top level"""
    lib = env.lib
    ns, g, B = N // 16, 8, 3
    vals, _ = images(ns, B, 32)
    ct = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
    x = lib.export_ciphertext(ct)
    out = lib.bootstrap_many(ct, ns)
    p = pack(env.orc, env.trace(x, ns, True), g)
    assert p.shape[0] == 1
    ref, rsc = env.orc.bootstrap(env.boot, env.circ, env.keys, p[0], 0, 2.0 ** 40)
    exp = env.trace(unpack(env.orc, ref[None], g, B), ns, False)
    assert np.array_equal(lib.export_ciphertext(out), exp)
    assert lib.GetCiphertextScaleF(out) == float(rsc)
    delete(lib, [ct, out])


def test_bootstrap_many_runs_the_full_slot_circuit_at_batch_h(env):
    lib = env.lib
    ns = N // 16
    vals, _ = images(ns, 8, 33)
    ct8 = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
    ct1 = lib.slice_ciphertext(ct8, 0, 1)
    made = [lib.bootstrap_many(ct8, ns), lib.Bootstrap(ct1, FULL)]  # (tables: first use at this batch)
    hm, PM = profiled(lib, lambda: lib.bootstrap_many(ct8, ns))
    h1, P1 = profiled(lib, lambda: lib.Bootstrap(ct1, FULL))
    assert PM["lt_bsgs"]["launches"] == P1["lt_bsgs"]["launches"] > 0, (PM["lt_bsgs"], P1["lt_bsgs"])
    assert PM["lt_bsgs"]["bytes"] == P1["lt_bsgs"]["bytes"] > 0, (PM["lt_bsgs"], P1["lt_bsgs"])
    assert PM["mono_pack"]["launches"] == 1 and PM["mono_unpack"]["launches"] == 1, PM
    assert P1["mono_pack"]["launches"] == 0 and P1["mono_unpack"]["launches"] == 0, P1
    delete(lib, [ct8, ct1, hm, h1] + made)


@pytest.mark.parametrize("dense", [False, True])
def test_bootstrap_many_precision(env, dense):
    """8 images with N/16 slots (g = 8), supported on the first slots or dense, each refreshed image against
    the cleartext slot sums: the plain Bootstrap(ct, slots) within test_bootstrap_parity's 1e-6, and
    bootstrap_many within 4 x the plain call's max error (the margin of test_bootstrap_packed_precision; on
    the CPU oracle the ratio is 1.54 for supported inputs and 0.99 for dense ones).
    Measured on an MI355X, the worst of the eight images: supported inputs plain 1.68e-7, many 1.58e-7 (ratio
    0.94); dense inputs plain 1.96e-7, many 1.87e-7 (ratio 0.95)."""
    lib = env.lib
    ns = N // 16
    vals, exp = images(ns, 8, 34 + dense, dense)
    ct = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
    plain, many = lib.Bootstrap(ct, ns), lib.bootstrap_many(ct, ns)
    assert meta(lib, plain) == meta(lib, many)
    e_plain = np.abs(lib.decode_f64(lib.Decrypt(plain)) - exp).max(axis=1)
    e_many = np.abs(lib.decode_f64(lib.Decrypt(many)) - exp).max(axis=1)
    print("bootstrap %s inputs max |error|: plain %.3g many %.3g (ratio %.2f)" % (
        "dense" if dense else "supported", e_plain.max(), e_many.max(), e_many.max() / e_plain.max()))
    assert e_plain.max() < 1e-6  # test_bootstrap_parity's bar
    assert e_many.max() <= 4 * e_plain.max(), (e_many, e_plain)
    delete(lib, [ct, plain, many])


def test_complex_packed_bootstrap_many_refreshes_sixteen_images_in_one_circuit_run(env):
    """pack_complex, bootstrap_many, unpack_complex on 2 x 8 real images with N/16 slots: the circuit runs at
    batch 1 and every image decrypts; max error <= 4 x that of the plain Bootstrap of the same images (the
    unpacked images come back at twice the scale, which the decoder divides out).  Measured on an MI355X:
    plain 1.8e-7, packed 2.41e-7 (ratio 1.34)."""
    lib = env.lib
    ns = N // 16
    va, exp_a = images(ns, 8, 36)
    vb, exp_b = images(ns, 8, 37)
    a, b = (lib.Encrypt(lib.encode_batch(v, 0, 1 << 40)) for v in (va, vb))
    one = lib.slice_ciphertext(a, 0, 1)
    made = [lib.Bootstrap(one, FULL)]
    z = lib.pack_complex(a, b)
    r, PM = profiled(lib, lambda: lib.bootstrap_many(z, ns))
    h1, P1 = profiled(lib, lambda: lib.Bootstrap(one, FULL))
    assert PM["lt_bsgs"]["launches"] == P1["lt_bsgs"]["launches"] > 0
    assert PM["lt_bsgs"]["bytes"] == P1["lt_bsgs"]["bytes"] > 0
    re, im = lib.unpack_complex(r)
    pa, pb = lib.Bootstrap(a, ns), lib.Bootstrap(b, ns)
    assert lib.GetCiphertextScaleF(re) == lib.GetCiphertextScaleF(im) == 2 * lib.GetCiphertextScaleF(pa)

    def err(h, e):
        return float(np.abs(lib.decode_f64(lib.Decrypt(h)) - e).max())

    plain, packed = max(err(pa, exp_a), err(pb, exp_b)), max(err(re, exp_a), err(im, exp_b))
    print("16 images, one circuit run: max |error| plain %.3g packed %.3g (ratio %.2f)" % (
        plain, packed, packed / plain))
    assert plain < 1e-6
    assert packed <= 4 * plain, (packed, plain)
    delete(lib, [a, b, one, z, r, h1, re, im, pa, pb] + made)


# ---- 4. graph capture ----------------------------------------------------------------------------
def test_captured_pack_unpack_and_trace_replay_to_the_same_bits(env):
    lib = env.lib
    a = lib.import_ciphertext(rand_ct(np.random.default_rng(40), env.mods, TOP, N, B=3), SCALE)
    wt = lib.slot_trace_new(a, N // 16, mean=True)
    wp = lib.pack_monomials(wt, 8)
    wu = lib.unpack_monomials(wp, 8, 3)
    eager = [lib.export_ciphertext(h) for h in (wt, wp, wu)]
    lib.OrionHipGraphBegin()
    try:
        t = lib.slot_trace_new(a, N // 16, mean=True)
        p = lib.pack_monomials(t, 8)
        u = lib.unpack_monomials(p, 8, 3)
    finally:
        gid = lib.OrionHipGraphEnd()
    for _ in range(2):
        assert lib.OrionHipGraphLaunch(gid) == 0
        lib.OrionHipSynchronize()
        for h, e in zip((t, p, u), eager):
            assert np.array_equal(lib.export_ciphertext(h), e)
    lib.OrionHipGraphDestroy(gid)
    delete(lib, [a, wt, wp, wu, t, p, u])


# ---- 5. pipelines --------------------------------------------------------------------------------
def test_pipeline_thread_runs_every_call_on_the_schemes_operands(env):
    lib = env.lib
    ns = N // 16
    vals, _ = images(ns, 3, 50)
    ct = lib.Encrypt(lib.encode_batch(vals, 1, 1 << 40))

    def work_on(lib):
        t = lib.slot_trace_new(ct, ns, mean=True)
        p = lib.pack_monomials(t, 8)
        u = lib.unpack_monomials(p, 8, 3)
        bm = lib.bootstrap_many(ct, ns)
        hs = [t, p, u, bm]
        bits = [lib.export_ciphertext(h) for h in hs]
        delete(lib, hs)
        return hs, bits

    _, exp = work_on(lib)
    peer = lib.OrionHipPeerCreate()
    assert peer >= 1
    res = {}

    def work():
        try:
            assert lib.OrionHipPeerSelect(peer) == 0
            res["handles"], res["bits"] = work_on(lib)
        except BaseException as e:  # reported below
            res["error"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "error" not in res, res["error"]
    assert all(h >> 20 == peer for h in res["handles"]), res["handles"]
    for got, e in zip(res["bits"], exp):
        assert np.array_equal(got, e)
    delete(lib, [ct])


# ---- 6. errors -----------------------------------------------------------------------------------
def test_errors_allocate_nothing(env):
    lib = env.lib
    x = rand_ct(np.random.default_rng(60), env.mods, 2, N, B=3)
    a = lib.import_ciphertext(x, SCALE)
    live, held = sorted(lib.GetLiveCiphertexts()), in_use(lib)
    unknown = max(live) + 1000

    def refused(match, fn, *args):
        with pytest.raises(RuntimeError, match=match):
            fn(*args)
        assert sorted(lib.GetLiveCiphertexts()) == live and in_use(lib) == held, match

    for fn in (lambda h: lib.pack_monomials(h, 8), lambda h: lib.unpack_monomials(h, 8, 3),
               lambda h: lib.slot_trace_new(h, N // 16), lambda h: lib.bootstrap_many(h, N // 16)):
        refused(f"handle not found: {unknown}", fn, unknown)
    for g in (0, -1, N + 1):
        refused(rf"g = {g} is out of range \[1, {N}\]", lib.pack_monomials, a, g)
        refused(rf"g = {g} is out of range \[1, {N}\]", lib.unpack_monomials, a, g, 3)
    for ns in (0, 1, 3, N // 2 + 1, N):
        refused(rf"slots must be a power of two in \[2, {N // 2}\]", lib.slot_trace_new, a, ns)
        refused(rf"slots must be a power of two in \[2, {N // 2}\]", lib.bootstrap_many, a, ns)
    # a batch of 3 holds the groups of 17..24 images at g = 8, of 3 at g = 1
    for g, B in ((8, 3), (8, 16), (8, 25), (1, 2), (8, 0), (8, -5)):
        refused(rf"cannot unpack {B} images at g = {g} from a batch of 3", lib.unpack_monomials, a, g, B)
    ok = lib.unpack_monomials(a, 8, 17)
    assert lib.GetCiphertextBatch(ok) == 17
    lib.OrionHipGraphBegin()
    try:
        cl = lib.CloneCiphertext(a)
        with pytest.raises(RuntimeError, match="OrionHipBootstrapMany is not allowed while capturing a graph"):
            lib.bootstrap_many(a, N // 16)
        assert sorted(lib.GetLiveCiphertexts()) == sorted(live + [ok, cl])
    finally:
        lib.OrionHipGraphDestroy(lib.OrionHipGraphEnd())
    delete(lib, [ok, cl])
    assert sorted(lib.GetLiveCiphertexts()) == live
    delete(lib, [a])


def test_fresh_scheme_refusals_allocate_nothing(torch_cuda):
    """on a scheme where none of the calls has run: a refused argument does not make the factor rows (the pool
    holds what it held); without the full-slot bootstrapper the message names N/2 and NewBootstrapper; and
    the three capturable calls, before their warm call, refuse an open capture (the factor rows and the
    Galois keys need a host synchronisation) and leave it usable"""
    lib = make_scheme(logq=SMALL["logq"], logp=SMALL["logp"], seed=61)
    try:
        a = lib.import_ciphertext(rand_ct(np.random.default_rng(61), lib.moduli(), 2, lib.N, B=2), SCALE)
        lib.NewBootstrapper(BTP_LOGP, N // 16)  # the sparse one does not serve
        lib.OrionHipSynchronize()
        live, held = sorted(lib.GetLiveCiphertexts()), in_use(lib)

        def refused(match, fn):
            with pytest.raises(RuntimeError, match=match):
                fn()
            assert sorted(lib.GetLiveCiphertexts()) == live and in_use(lib) == held, match

        refused("g = 0 is out of range", lambda: lib.pack_monomials(a, 0))
        refused("g = 0 is out of range", lambda: lib.unpack_monomials(a, 0, 2))
        refused("cannot unpack 5 images at g = 2 from a batch of 2", lambda: lib.unpack_monomials(a, 2, 5))
        refused(f"cannot unpack {2 ** 31 - 1} images at g = 1 from a batch of 2",
                lambda: lib.unpack_monomials(a, 1, 2 ** 31 - 1))
        refused("slots must be a power of two", lambda: lib.slot_trace_new(a, 3))
        refused(rf"N/2 = {N // 2} \(NewBootstrapper\(logPs, {N // 2}\)", lambda: lib.bootstrap_many(a, N // 16))
        lib.OrionHipGraphBegin()
        try:
            cl = lib.CloneCiphertext(a)
            for fn in (lambda: lib.pack_monomials(a, 2), lambda: lib.unpack_monomials(a, 2, 3),
                       lambda: lib.slot_trace_new(a, N // 4)):
                with pytest.raises(RuntimeError, match="needs a host synchronisation, not allowed while capturing"):
                    fn()
                assert sorted(lib.GetLiveCiphertexts()) == sorted(live + [cl])
        finally:
            gid = lib.OrionHipGraphEnd()
        assert lib.OrionHipGraphLaunch(gid) == 0
        lib.OrionHipSynchronize()
        assert np.array_equal(lib.export_ciphertext(cl), lib.export_ciphertext(a))
        lib.OrionHipGraphDestroy(gid)
        out = lib.unpack_monomials(lib.pack_monomials(a, 2), 2, 2)  # outside a capture the same calls go through
        assert lib.GetCiphertextBatch(out) == 2
    finally:
        lib.DeleteScheme()


def test_missing_key_without_the_secret_key(torch_cuda):
    """a scheme that imported a key bundle without the secret has the key of the rotation by N/8 and lacks
    the one by N/4: the trace over N/8 slots (g = 4) needs both and fails with Rotate's message and the
    element, before anything is allocated; so does the trace over N/4 slots, which needs only the missing
    one, and so does OrionHipBootstrapMany at either slot count, whose full-slot bootstrapper exists"""
    torch = torch_cuda
    lib = make_scheme(logq=SMALL["logq"], logp=SMALL["logp"], seed=62)
    try:
        lib.AddRotationKey(N // 8)
        n = lib.KeyBundleBytes(0)
        buf = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert lib.lib.ExportKeyBundle(buf.data_ptr(), 0) == 0
        lib.OrionHipSynchronize()
        lib.DeleteScheme()
        lib.new_scheme(SMALL["logn"], SMALL["logq"], SMALL["logp"], 40, h=192, seed=63)
        assert lib.lib.ImportKeyBundle(buf.data_ptr(), n) == 0, lib.lib.OrionHipLastError()
        x = lib.import_ciphertext(rand_ct(np.random.default_rng(62), lib.moduli(), 5, lib.N, B=2), SCALE)
        live, held = sorted(lib.GetLiveCiphertexts()), in_use(lib)
        with pytest.raises(RuntimeError, match="secret key not generated") as rot:
            lib.Rotate(x, N // 4)
        gel = int(lib.GaloisElement(N // 4))
        for ns in (N // 8, N // 4):
            with pytest.raises(RuntimeError, match=rf"galois key {gel} \(rotation by {N // 4}\)") as tr:
                lib.slot_trace_new(x, ns)
            assert str(rot.value).split(": ", 1)[1] in str(tr.value)  # Rotate's message
            assert sorted(lib.GetLiveCiphertexts()) == live and in_use(lib) == held
        lib.NewBootstrapper(BTP_LOGP, N // 2)  # (a scheme without the secret builds the circuit alone)
        lib.OrionHipSynchronize()
        held = in_use(lib)
        for ns in (N // 8, N // 4):
            with pytest.raises(RuntimeError, match=rf"galois key {gel} \(rotation by {N // 4}\)") as bm:
                lib.bootstrap_many(x, ns)
            assert str(rot.value).split(": ", 1)[1] in str(bm.value)
            assert sorted(lib.GetLiveCiphertexts()) == live and in_use(lib) == held
        r = lib.Rotate(x, N // 8)  # the key that exists serves
        assert r == x
    finally:
        lib.DeleteScheme()


def test_conjugate_invariant_ring_is_refused(torch_cuda):
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(13, [29] + [26] * 3, [29, 29], 26, ringtype="ConjugateInvariant", seed=64)
    try:
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        a = lib.import_ciphertext(rand_ct(np.random.default_rng(64), lib.moduli(), 2, lib.N), SCALE)
        live = sorted(lib.GetLiveCiphertexts())
        for fn in (lambda: lib.pack_monomials(a, 2), lambda: lib.unpack_monomials(a, 2, 2),
                   lambda: lib.slot_trace_new(a, 64), lambda: lib.bootstrap_many(a, 64)):
            with pytest.raises(RuntimeError, match="needs the Standard ring"):
                fn()
            assert sorted(lib.GetLiveCiphertexts()) == live
    finally:
        lib.DeleteScheme()


def test_poisoned_source_is_refused(torch_cuda):
    """an operand whose deferred rotate-and-add failed (an allocation past the pool cap, the recipe of
    test_deferred_rotation_failure_poisons): each call returns the poison and allocates nothing"""
    lib = make_scheme(logq=SMALL["logq"], logp=SMALL["logp"], seed=65)
    try:
        lib.AddRotationKey(1)
        rng = np.random.default_rng(65)
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
        for fn in (lambda: lib.pack_monomials(x, 2), lambda: lib.unpack_monomials(x, 2, 3),
                   lambda: lib.slot_trace_new(x, 64), lambda: lib.bootstrap_many(x, 64)):
            with pytest.raises(RuntimeError, match="deferred rotation by 1 failed"):
                fn()
            assert sorted(lib.GetLiveCiphertexts()) == live
        out = lib.pack_monomials(y, 2)  # with a sound operand the same call goes through
        assert lib.GetCiphertextLevel(out) == 5 and lib.GetCiphertextBatch(out) == 1
    finally:
        lib.DeleteScheme()
