"""Complex packing: OrionHipConjugateNew, OrionHipPackComplex,
OrionHipUnpackComplex and OrionHipBootstrapPacked (include/orion_hip.h;
pack_complex_kernel, unpack_complex_kernel, Context::bootstrap_packed).

The expectations are composed from oracle pieces only -- Oracle.ntt of the
unit vector at N/2 for I, Oracle.mul_coeffs, numpy sums mod q, Oracle.rotate
by 2N-1 with the exported conjugation key, Oracle.bootstrap -- and every
parity comparison is bit for bit.

One scheme serves the module: N = 2^13, residual chain [60] + [40] x 5, logP
[60, 60], bootstrapping P [61, 61], h = 192 (the shapes of
test_bootstrap_parity), with a full-slot and a sparse (N/16 slots)
bootstrapper."""
import threading

import numpy as np
import pytest

from tests.helpers import SMALL, SchemeCache, bootstrap_keys, bootstrap_oracle, rand_ct

pytestmark = pytest.mark.gpu

LOGN, LOGQ, LOGP, BTP_LOGP = 13, [60] + [40] * 5, [60, 60], [61, 61]
TOP = len(LOGQ) - 1
N = 1 << LOGN
CONJ = 2 * N - 1
SCALE = 2.0 ** 20  # of an imported operand: printed exactly by the error messages
SEED = 2718


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


class Env:
    def __init__(self, oracle_mod):
        self.oracle_mod = oracle_mod
        self.lib = make_scheme()
        self.mods = self.lib.moduli()
        self.orc = oracle_mod.Oracle(LOGN, self.mods, len(LOGQ), len(LOGP))
        unit = np.zeros(N, dtype=np.uint64)
        unit[N // 2] = 1
        self.I = np.stack([self.orc.ntt(j, unit) for j in range(TOP + 1)])  # the NTT of X^(N/2), limb by limb
        # the conjugation key, made for the top level by the first call (it covers every level below)
        x = self.lib.import_ciphertext(rand_ct(np.random.default_rng(1), self.mods, TOP, N), SCALE)
        y = self.lib.conjugate_new(x)
        self.gk = self.lib.export_galois_key(CONJ)
        delete(self.lib, [x, y])
        self.btp = {}

    def q(self, level):
        return np.array(self.mods[:level + 1], dtype=np.uint64)[:, None]

    def mul_i(self, x):
        """I o x for x [..][limbs][N]"""
        nl = x.shape[-2]
        flat = x.reshape(-1, nl, N)
        return np.stack([self.orc.mul_coeffs(r, self.I[:nl], list(range(nl))) for r in flat]).reshape(x.shape)

    def pack(self, a, b):
        """a + I o b on the limbs both have: [B][2][level + 1][N]"""
        nl = min(a.shape[2], b.shape[2])
        return (a[:, :, :nl] + self.mul_i(b[:, :, :nl])) % self.q(nl - 1)  # residues below 2^61: the sum fits

    def conj(self, x):
        lv = x.shape[2] - 1
        return np.stack([self.orc.rotate(x[i], CONJ, self.gk, lv) for i in range(x.shape[0])])

    def unpack(self, x):
        """(x + yc, I o (yc - x)) with yc = sigma_{2N-1}(x)"""
        q = self.q(x.shape[2] - 1)
        yc = self.conj(x)
        return (x + yc) % q, self.mul_i((yc + (q - x)) % q)

    def bootstrapper(self, sparse):
        """(slot count, bootstrapping-chain oracle, circuit) of the full or the sparse bootstrapper.  Both are
        made and run once at the first call: they share the Galois keys of one bootstrapping chain, and a key
        made again for a higher level is a new key, so the keys are exported only after both have run"""
        if not self.btp:
            warm = self.lib.Encrypt(self.lib.encode_batch(np.zeros((2, N // 2), dtype=np.float32), 0, 1 << 40))
            for ns in (N // 2, N // 16):
                self.lib.NewBootstrapper(BTP_LOGP, ns)
                delete(self.lib, [self.lib.Bootstrap(warm, ns)])  # every key made at the level it ends at
            delete(self.lib, [warm])
            for ns in (N // 2, N // 16):
                self.btp[ns] = (ns,) + bootstrap_oracle(self.oracle_mod, self.lib, LOGN, 40, ns, BTP_LOGP)
        return self.btp[N // 16 if sparse else N // 2]


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


def launches(prof):
    return {k: v["launches"] for k, v in prof.items()}


def images(sparse, B, seed):
    """B real images uniform in (-1, 1) (zero from the sparse slot count on) and what a bootstrap returns for them"""
    ns = N // 16 if sparse else N // 2
    vals = np.random.default_rng(seed).uniform(-1, 1, (B, N // 2)).astype(np.float32)
    vals[:, ns:] = 0
    return vals, np.tile(vals[:, :ns], (1, N // 2 // ns)).astype(np.float64)


# ---- 1. conjugation ------------------------------------------------------------------------------
def test_conjugate_matches_the_oracle_rotation(env):
    lib = env.lib
    rng = np.random.default_rng(10)
    for level in (TOP, 0):
        x = rand_ct(rng, env.mods, level, N, B=2)
        h = lib.import_ciphertext(x, SCALE)
        c = lib.conjugate_new(h)
        assert (lib.GetCiphertextLevel(c), lib.GetCiphertextBatch(c), lib.GetCiphertextScaleF(c)) == (level, 2, SCALE)
        assert np.array_equal(lib.export_ciphertext(c), env.conj(x)), level
        delete(lib, [h, c])


def test_conjugate_twice_decrypts_to_the_input(env):
    lib = env.lib
    vals = np.random.default_rng(11).uniform(-1, 1, (2, N // 2)).astype(np.float32)
    ct = lib.Encrypt(lib.encode_batch(vals, TOP, 1 << 40))
    c1 = lib.conjugate_new(ct)
    c2 = lib.conjugate_new(c1)
    # the bar of test_bootstrap_parity for a fresh scale-2^40 encryption; a key switch adds noise of that order
    assert np.abs(lib.decode_f64(lib.Decrypt(c2)) - vals).max() < 1e-6
    # a real image is its own conjugate
    assert np.abs(lib.decode_f64(lib.Decrypt(c1)) - vals).max() < 1e-6
    delete(lib, [ct, c1, c2])


# ---- 2. pack -------------------------------------------------------------------------------------
def run_pack(env, a, b, same=False):
    lib = env.lib
    ha = lib.import_ciphertext(a, SCALE)
    hb = ha if same else lib.import_ciphertext(b, SCALE)
    out = lib.pack_complex(ha, hb)
    exp = env.pack(a, a if same else b)
    assert lib.GetCiphertextLevel(out) == exp.shape[2] - 1 and lib.GetCiphertextBatch(out) == exp.shape[0]
    assert lib.GetCiphertextScaleF(out) == SCALE
    got = lib.export_ciphertext(out)
    assert np.array_equal(got, exp)
    delete(lib, [ha, hb, out])
    return got


@pytest.mark.parametrize("B,la,lb", [(1, TOP, TOP), (1, TOP, 2), (3, TOP, TOP), (3, 2, TOP), (64, 1, 1), (64, 2, 1)])
def test_pack_matches_the_composition(env, B, la, lb):
    rng = np.random.default_rng(20 + B + la)
    got = run_pack(env, rand_ct(rng, env.mods, la, N, B=B), rand_ct(rng, env.mods, lb, N, B=B))
    assert got.shape[:3] == (B, 2, min(la, lb) + 1)


def test_pack_of_a_handle_with_itself(env):
    a = rand_ct(np.random.default_rng(21), env.mods, TOP, N, B=2)
    run_pack(env, a, None, same=True)


def test_pack_planted_maxima(env):
    """every residue of both operands is q_j - 1: the product and the sum wrap on every coefficient"""
    top = np.zeros((2, 2, TOP + 1, N), dtype=np.uint64)
    for j in range(TOP + 1):
        top[:, :, j, :] = env.mods[j] - 1
    run_pack(env, top, top.copy())


# ---- 3. unpack -----------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [TOP, 0])
def test_unpack_matches_the_composition(env, level):
    lib = env.lib
    x = rand_ct(np.random.default_rng(30 + level), env.mods, level, N, B=3)
    for j in range(level + 1):  # planted: both differences wrap
        x[0, :, j, :16] = env.mods[j] - 1
        x[1, :, j, :16] = 0
    h = lib.import_ciphertext(x, SCALE)
    re, im = lib.unpack_complex(h)
    ere, eim = env.unpack(x)
    for got, exp in ((re, ere), (im, eim)):
        assert (lib.GetCiphertextLevel(got), lib.GetCiphertextBatch(got)) == (level, 3)
        assert lib.GetCiphertextScaleF(got) == 2 * SCALE  # exactly twice the input's
        assert np.array_equal(lib.export_ciphertext(got), exp)
    delete(lib, [h, re, im])


def test_unpack_of_pack_decrypts_to_both_images(env):
    lib = env.lib
    vals = np.random.default_rng(31).uniform(-1, 1, (2, 2, N // 2)).astype(np.float32)
    a, b = (lib.Encrypt(lib.encode_batch(v, TOP, 1 << 40)) for v in vals)
    z = lib.pack_complex(a, b)
    re, im = lib.unpack_complex(z)
    assert lib.GetCiphertextScaleF(re) == lib.GetCiphertextScaleF(im) == 2.0 ** 41
    err = [float(np.abs(lib.decode_f64(lib.Decrypt(h)) - v).max()) for h, v in ((re, vals[0]), (im, vals[1]))]
    print("unpack(pack(a, b)) max |error| re %.3g im %.3g" % tuple(err))
    # the bar test_bootstrap_parity uses for a fresh scale-2^40 encryption
    assert max(err) < 1e-6, err
    delete(lib, [a, b, z, re, im])


# ---- 4. launch counts ----------------------------------------------------------------------------
def test_pack_is_one_elementwise_launch_and_unpack_one_more_than_a_conjugation(env):
    lib = env.lib
    rng = np.random.default_rng(40)
    a, b = (lib.import_ciphertext(rand_ct(rng, env.mods, TOP, N, B=2), SCALE) for _ in range(2))
    made = []
    z, P = profiled(lib, lambda: lib.pack_complex(a, b))
    P = launches(P)
    assert P["elementwise"] == 1 and sum(P.values()) == 1, P
    made.append(lib.conjugate_new(z))  # (tables: first use at this batch)
    c, C = profiled(lib, lambda: lib.conjugate_new(z))
    (re, im), U = profiled(lib, lambda: lib.unpack_complex(z))
    C, U = launches(C), launches(U)
    # the conjugate is stored, then one kernel reads it and ct once and writes both outputs
    assert U["elementwise"] == C["elementwise"] + 1, (U, C)
    for k in C:
        if k != "elementwise":
            assert U[k] == C[k], (k, U, C)
    delete(lib, [a, b, z, c, re, im] + made)


# ---- 5. real-linear layers -----------------------------------------------------------------------
def test_linear_transform_acts_on_both_images(env):
    """One transform with diagonals {0, 3} (the recipe of test_bootstrap_functional) on Pack(a, b), rescaled
    and unpacked, against the same transform on a and on b separately; all decrypted and compared with the
    float64 result.  Bar: packed max error <= 4 x the separate path's on the same inputs (the separate path is
    the existing behaviour; the factor covers the spread of two noise maxima and the sqrt(2) larger packed
    message).  Measured on an MI355X: separate 8.1e-8, packed 1.3e-7 (ratio 1.6)."""
    lib = env.lib
    rng = np.random.default_rng(50)
    n = N // 2
    vals = rng.uniform(-1, 1, (2, 2, n)).astype(np.float32)
    idx = [0, 3]
    diags = rng.uniform(-1, 1, (2, n)).astype(np.float32)
    lt = lib.GenerateLinearTransform(idx, list(diags.reshape(-1)), 3, 2.0, "none")
    a, b = (lib.Encrypt(lib.encode_batch(v, 3, 1 << 40)) for v in vals)
    exp = [sum(diags[i].astype(np.float64) * np.roll(v, -d, axis=1) for i, d in enumerate(idx)) for v in vals]

    def apply(ct):
        y = lib.EvaluateLinearTransform(lt, ct)
        lib.Rescale(y)
        return y

    def err(h, e):
        return float(np.abs(lib.decode_f64(lib.Decrypt(h)) - e).max())

    ya, yb = apply(a), apply(b)
    z = lib.pack_complex(a, b)
    yz = apply(z)
    re, im = lib.unpack_complex(yz)
    sep, packed = max(err(ya, exp[0]), err(yb, exp[1])), max(err(re, exp[0]), err(im, exp[1]))
    print("linear transform max |error|: separate %.3g packed %.3g" % (sep, packed))
    assert sep < 1e-3  # test_bootstrap_functional's bar for this transform
    assert packed <= 4 * sep, (packed, sep)
    delete(lib, [a, b, ya, yb, z, yz, re, im])
    lib.DeleteLinearTransform(lt)


# ---- 6. OrionHipBootstrapPacked ------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_bootstrap_packed_equals_the_public_composition(env, sparse):
    """B = 4: Slice, Slice, Pack, Bootstrap, Unpack, Stack.  B = 3: image 0 rides with image 2, image 1 alone
    equals Unpack(Bootstrap(slice))[0]"""
    lib = env.lib
    ns = env.bootstrapper(sparse)[0]
    vals, _ = images(sparse, 4, 60 + sparse)
    ct = lib.Encrypt(lib.encode_batch(vals, 2, 1 << 40))  # above level 0: only limb 0 is read
    out = lib.bootstrap_packed(ct, ns)
    lo, hi = lib.slice_ciphertext(ct, 0, 2), lib.slice_ciphertext(ct, 2, 2)
    z = lib.pack_complex(lo, hi)
    r = lib.Bootstrap(z, ns)
    re, im = lib.unpack_complex(r)
    comp = lib.stack_ciphertexts([re, im])
    assert (lib.GetCiphertextLevel(out), lib.GetCiphertextBatch(out)) == (TOP, 4)
    assert lib.GetCiphertextScaleF(out) == lib.GetCiphertextScaleF(comp) == 2 * lib.GetCiphertextScaleF(r)
    assert np.array_equal(lib.export_ciphertext(out), lib.export_ciphertext(comp))
    # B = 3
    ct3 = lib.slice_ciphertext(ct, 0, 3)
    out3 = lib.bootstrap_packed(ct3, ns)
    assert (lib.GetCiphertextLevel(out3), lib.GetCiphertextBatch(out3)) == (TOP, 3)
    got3 = lib.export_ciphertext(out3)
    s0, s1, s2 = (lib.slice_ciphertext(ct, i, 1) for i in range(3))
    z02 = lib.pack_complex(s0, s2)
    r02, r1 = lib.Bootstrap(z02, ns), lib.Bootstrap(s1, ns)
    re02, im02 = lib.unpack_complex(r02)
    re1, im1 = lib.unpack_complex(r1)
    assert np.array_equal(got3[0], lib.export_ciphertext(re02)[0])
    assert np.array_equal(got3[1], lib.export_ciphertext(re1)[0])
    assert np.array_equal(got3[2], lib.export_ciphertext(im02)[0])
    delete(lib, [ct, out, lo, hi, z, r, re, im, comp, ct3, out3, s0, s1, s2, z02, r02, r1, re02, im02, re1, im1])


@pytest.mark.parametrize("sparse", [False, True])
def test_bootstrap_packed_matches_the_oracle(env, sparse):
    """one pair: Oracle.bootstrap of the composed packed level-0 ciphertext, then the composed unpack at the
    top level.  B = 1 is Bootstrap followed by ct + conj ct at twice the scale"""
    lib = env.lib
    ns, boot, circ = env.bootstrapper(sparse)
    vals, _ = images(sparse, 2, 62 + sparse)
    ct = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
    x = lib.export_ciphertext(ct)
    out = lib.bootstrap_packed(ct, ns)
    got = lib.export_ciphertext(out)
    keys = bootstrap_keys(lib, ns)
    packed0 = env.pack(x[:1], x[1:])
    ref, rsc = env.orc.bootstrap(boot, circ, keys, packed0[0], 0, 2.0 ** 40)
    re, im = env.unpack(ref[None])
    assert np.array_equal(got[0], re[0]) and np.array_equal(got[1], im[0])
    assert lib.GetCiphertextScaleF(out) == 2 * float(rsc)
    one = lib.slice_ciphertext(ct, 0, 1)
    out1, plain = lib.bootstrap_packed(one, ns), lib.Bootstrap(one, ns)
    p = lib.export_ciphertext(plain)
    assert np.array_equal(lib.export_ciphertext(out1), (p + env.conj(p)) % env.q(TOP))
    assert lib.GetCiphertextScaleF(out1) == 2 * lib.GetCiphertextScaleF(plain)
    delete(lib, [ct, out, one, out1, plain])


@pytest.mark.parametrize("sparse", [False, True])
def test_bootstrap_packed_precision(env, sparse):
    """each refreshed image against the cleartext: max error <= 4 x the max error of the plain Bootstrap of
    the same images (on the CPU oracle the ratio is 2.0 for full slots and 1.1 for sparse ones; doubling the
    coefficients gives the cubic EvalMod term 8 x at worst, and random slots are far from that).  Measured on
    an MI355X, the worst of the four images: full slots plain 1.05e-7, packed 1.66e-7 (ratio 1.6); sparse
    slots plain 1.87e-7, packed 2.52e-7 (ratio 1.35)."""
    lib = env.lib
    ns = env.bootstrapper(sparse)[0]
    vals, exp = images(sparse, 4, 64 + sparse)
    ct = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
    plain, packed = lib.Bootstrap(ct, ns), lib.bootstrap_packed(ct, ns)
    e_plain = np.abs(lib.decode_f64(lib.Decrypt(plain)) - exp).max(axis=1)
    e_packed = np.abs(lib.decode_f64(lib.Decrypt(packed)) - exp).max(axis=1)
    print("bootstrap %s slots max |error| per image: plain %s packed %s" % (
        "sparse" if sparse else "full", ["%.3g" % e for e in e_plain], ["%.3g" % e for e in e_packed]))
    assert e_plain.max() < 1e-6  # test_bootstrap_parity's bar
    assert e_packed.max() <= 4 * e_plain.max(), (e_packed, e_plain)
    delete(lib, [ct, plain, packed])


@pytest.mark.parametrize("sparse", [False, True])
def test_bootstrap_packed_runs_the_circuit_at_half_the_batch(env, sparse):
    lib = env.lib
    ns = env.bootstrapper(sparse)[0]
    vals, _ = images(sparse, 4, 66 + sparse)
    ct4 = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
    ct2 = lib.slice_ciphertext(ct4, 0, 2)
    made = [lib.bootstrap_packed(ct4, ns), lib.Bootstrap(ct2, ns)]  # (tables: first use at this batch)
    h4, P4 = profiled(lib, lambda: lib.bootstrap_packed(ct4, ns))
    h2, P2 = profiled(lib, lambda: lib.Bootstrap(ct2, ns))
    assert P4["lt_bsgs"]["launches"] == P2["lt_bsgs"]["launches"] > 0, (P4["lt_bsgs"], P2["lt_bsgs"])
    assert P4["lt_bsgs"]["bytes"] == P2["lt_bsgs"]["bytes"] > 0, (P4["lt_bsgs"], P2["lt_bsgs"])
    delete(lib, [ct4, ct2, h4, h2] + made)


# ---- 7. graph capture ----------------------------------------------------------------------------
def test_captured_pack_and_unpack_replay_to_the_same_bits(env):
    lib = env.lib
    rng = np.random.default_rng(70)
    a, b = (lib.import_ciphertext(rand_ct(rng, env.mods, TOP, N, B=2), SCALE) for _ in range(2))
    wz = lib.pack_complex(a, b)
    wre, wim = lib.unpack_complex(wz)
    eager = [lib.export_ciphertext(h) for h in (wz, wre, wim)]
    lib.OrionHipGraphBegin()
    try:
        z = lib.pack_complex(a, b)
        re, im = lib.unpack_complex(z)
    finally:
        gid = lib.OrionHipGraphEnd()
    for _ in range(2):
        assert lib.OrionHipGraphLaunch(gid) == 0
        lib.OrionHipSynchronize()
        for h, e in zip((z, re, im), eager):
            assert np.array_equal(lib.export_ciphertext(h), e)
    lib.OrionHipGraphDestroy(gid)
    delete(lib, [a, b, wz, wre, wim, z, re, im])


# ---- 8. pipelines --------------------------------------------------------------------------------
def test_pipeline_thread_packs_bootstraps_and_unpacks_the_schemes_operands(env):
    lib = env.lib
    ns = env.bootstrapper(True)[0]
    vals, _ = images(True, 2, 80)
    ct = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
    a, b = lib.slice_ciphertext(ct, 0, 1), lib.slice_ciphertext(ct, 1, 1)

    def work_on(lib):
        z = lib.pack_complex(a, b)
        re, im = lib.unpack_complex(z)
        bp = lib.bootstrap_packed(ct, ns)
        hs = [z, re, im, bp]
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
    delete(lib, [ct, a, b])


# ---- 9. errors -----------------------------------------------------------------------------------
def test_errors_allocate_nothing(env):
    from orion_amd.backend import c_int
    lib = env.lib
    env.bootstrapper(True)
    rng = np.random.default_rng(90)
    x = rand_ct(rng, env.mods, 2, N, B=2)
    a, b = (lib.import_ciphertext(x, SCALE) for _ in range(2))
    three = lib.import_ciphertext(np.concatenate([x, x[:1]]), SCALE)
    scaled = lib.import_ciphertext(x, SCALE)
    lib.SetCiphertextScale(scaled, 2 ** 21)
    live = sorted(lib.GetLiveCiphertexts())
    unknown = max(live) + 1000

    def refused(match, fn, *args):
        with pytest.raises(RuntimeError, match=match):
            fn(*args)
        assert sorted(lib.GetLiveCiphertexts()) == live, match

    for fn in (lib.conjugate_new, lib.unpack_complex, lambda h: lib.pack_complex(a, h),
               lambda h: lib.pack_complex(h, a), lambda h: lib.bootstrap_packed(h, N // 16)):
        refused(f"handle not found: {unknown}", fn, unknown)
    refused(rf"{a} \(batch 2\) and {three} \(batch 3\): the batches differ", lib.pack_complex, a, three)
    refused(rf"{a} \(scale 1048576\) and {scaled} \(scale 2097152\): the scales differ", lib.pack_complex, a, scaled)
    out2 = (c_int * 2)(-7, -7)
    assert lib.lib.OrionHipUnpackComplex(a, None) == -1 and b"null" in lib.lib.OrionHipLastError()
    assert lib.lib.OrionHipUnpackComplex(unknown, out2) == -1 and list(out2) == [-7, -7]
    assert sorted(lib.GetLiveCiphertexts()) == live
    refused("no bootstrapper found for slot count: 64", lib.bootstrap_packed, a, 64)
    delete(lib, [a, b, three, scaled])


def test_conjugate_invariant_ring_is_refused(torch_cuda):
    from orion_amd.backend import HipLibrary, c_int
    lib = HipLibrary().new_scheme(13, [29] + [26] * 3, [29, 29], 26, ringtype="ConjugateInvariant", seed=91)
    try:
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        a = lib.import_ciphertext(rand_ct(np.random.default_rng(91), lib.moduli(), 2, lib.N), SCALE)
        live = sorted(lib.GetLiveCiphertexts())
        for fn in (lambda: lib.conjugate_new(a), lambda: lib.pack_complex(a, a), lambda: lib.unpack_complex(a),
                   lambda: lib.bootstrap_packed(a, 64)):
            with pytest.raises(RuntimeError, match="complex packing needs the Standard ring"):
                fn()
            assert sorted(lib.GetLiveCiphertexts()) == live
        out2 = (c_int * 2)(-7, -7)
        assert lib.lib.OrionHipUnpackComplex(a, out2) == -1 and list(out2) == [-7, -7]
    finally:
        lib.DeleteScheme()


def test_poisoned_source_is_refused(torch_cuda):
    """an operand whose deferred rotate-and-add failed (an allocation past the pool cap, the recipe of
    test_deferred_rotation_failure_poisons): each call returns the poison and allocates nothing"""
    lib = make_scheme(logq=SMALL["logq"], logp=SMALL["logp"], seed=92)
    try:
        lib.AddRotationKey(1)
        rng = np.random.default_rng(92)
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
        for fn in (lambda: lib.conjugate_new(x), lambda: lib.pack_complex(y, x), lambda: lib.pack_complex(x, y),
                   lambda: lib.unpack_complex(x), lambda: lib.bootstrap_packed(x, 64)):
            with pytest.raises(RuntimeError, match="deferred rotation by 1 failed"):
                fn()
            assert sorted(lib.GetLiveCiphertexts()) == live
        out = lib.pack_complex(y, y)  # with sound operands the same call goes through
        assert lib.GetCiphertextLevel(out) == 5
    finally:
        lib.DeleteScheme()


# ---- the circuit's own multiplication by i ---------------------------------------------------------
def test_exported_monomial_is_the_transform_of_the_monomial(env):
    """the full-slot circuit multiplies by i with the packing kernels' constant and holds no plaintext for it;
    bootstrap_export("mono_i") still answers with the NTT of X^(N/2) over the bootstrapping chain's Q primes,
    limb by limb the oracle's forward transform, and a sparse circuit (which never multiplies by i) refuses"""
    lib = env.lib
    ns, boot, _ = env.bootstrapper(False)
    nq = len(lib.bootstrap_moduli(ns)[0])
    unit = np.zeros(N, dtype=np.uint64)
    unit[N // 2] = 1
    got = lib.bootstrap_export(ns, "mono_i")
    assert got.shape == (nq * N,)
    for j in range(nq):
        assert np.array_equal(got[j * N:(j + 1) * N], boot.ntt(j, unit)), j
    with pytest.raises(RuntimeError, match=r"sparse-slot circuit: no X\^\(N/2\) plaintext"):
        lib.bootstrap_export(env.bootstrapper(True)[0], "mono_i")
