"""A ModDown whose result is rescaled by the next call runs as one division by
P q_l (backend.hip Context::moddown_rescale, reached through the "ModDown
pending" deferral behind the unchanged C-ABI).  Every test compares bit for
bit: against the CPU oracle's sequential ModDown -> rescale, and against the
same calls on a scheme made with ORION_DEFER=0, which runs them op by op."""
import threading

import numpy as np
import pytest

from tests.helpers import SMALL, rand_ct, plant_runs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


SEED = 2718


def scheme(monkeypatch, defer, logn=SMALL["logn"], logq=SMALL["logq"], logp=SMALL["logp"], ringtype="standard"):
    """A scheme with the library's deferral on or off (read when it is made);
    the same seed gives both the same keys."""
    from orion_amd.backend import HipLibrary
    monkeypatch.setenv("ORION_DEFER", "1" if defer else "0")
    lib = HipLibrary().new_scheme(logn, logq, logp, 40, h=192, seed=SEED, ringtype=ringtype)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    lib.GenerateRelinearizationKey()
    return lib


def profiled(lib, fn):
    lib.OrionHipProfileReset()
    lib.OrionHipProfile(1)
    r = fn()
    lib.OrionHipProfile(0)
    p = lib.profile_read()
    return r, {k: p[k]["launches"] for k in p}


def assert_merged(pm, pu, copies=0):
    """the merged run against the op-by-op run: one forward NTT (the ModDown's,
    which only fed the rescale) and one inverse NTT (limb l rides with the P
    limbs) fewer, the same basis_ext launches, nothing else changed (copies:
    with the deferral off RescaleNew copies its result at once)"""
    assert pm["ntt_fwd"] == pu["ntt_fwd"] - 1, (pm, pu)
    assert pm["ntt_inv"] == pu["ntt_inv"] - 1, (pm, pu)
    assert pm["basis_ext"] == pu["basis_ext"] and pm["basis_ext"] >= 1, (pm, pu)
    assert pm["elementwise"] == pu["elementwise"] - copies, (pm, pu)
    for k in pu:
        if k not in ("ntt_fwd", "ntt_inv", "elementwise"):
            assert pm[k] == pu[k], (k, pm, pu)


# the top level with B = 8, and level 1 (one output limb) with B = 32: in both
# nc B (level + 1) > 64, so no launch is small enough for the fused latency path
SHAPES = [(len(SMALL["logq"]) - 1, 8), (1, 32)]
LT_IDX = [0, 1, 2, 3, 17, 64, 65, 300]


@pytest.mark.parametrize("level,B", SHAPES)
def test_linear_transform_then_rescale(torch_cuda, oracle_mod, monkeypatch, level, B):
    """EvaluateLinearTransform -> RescaleNew: the oracle's lt_bsgs followed by
    its rescale, the op-by-op library, and the launch counts."""
    rng = np.random.default_rng(100 * level + B)
    slots = (1 << SMALL["logn"]) // 2
    idx = LT_IDX + [slots - 1]
    diags = rng.uniform(-1, 1, (len(idx), slots)).astype(np.float32)
    res = {}
    x = None
    for defer in (False, True):
        lib = scheme(monkeypatch, defer)
        mods = lib.moduli()
        if x is None:
            x = plant_runs(rand_ct(rng, mods, level, lib.N, B=B), mods)
        lt = lib.GenerateLinearTransform(idx, list(diags.reshape(-1)), level, 2.0, "none")
        gels = lib.GetLinearTransformRotationKeys(lt)
        lib.GenerateConsolidatedRotationKeys(gels)
        ct = lib.import_ciphertext(x, 2.0 ** 40)
        lib.export_ciphertext(lib.RescaleNew(lib.EvaluateLinearTransform(lt, ct)))  # (tables, plans: first use)

        def run():
            out = lib.EvaluateLinearTransform(lt, ct)
            return out, lib.RescaleNew(out)

        (out, y), prof = profiled(lib, run)
        assert lib.GetCiphertextLevel(out) == level - 1 and lib.GetCiphertextLevel(y) == level - 1
        assert lib.GetCiphertextScaleF(y) == lib.GetCiphertextScaleF(out)
        got = lib.export_ciphertext(y)
        assert np.array_equal(lib.export_ciphertext(out), got)  # RescaleNew: the input rescaled, and a copy
        res[defer] = (got, prof)
        if defer:
            orc = oracle_mod.Oracle(SMALL["logn"], mods, len(SMALL["logq"]), len(SMALL["logp"]))
            pts = [lib.export_lt_diagonal(lt, d, level) for d in idx]
            gkeys = {g: lib.export_galois_key(g) for g in gels if g != 1}
            N1 = lib.GetLinearTransformN1(lt)
            for b in (0, B - 1):
                ref = orc.rescale(orc.lt_bsgs(x[b], level, idx, pts, N1, gkeys), level)
                assert np.array_equal(got[b], ref), b
        lib.DeleteScheme()
    assert np.array_equal(res[True][0], res[False][0])
    assert_merged(res[True][1], res[False][1], copies=1)


@pytest.mark.parametrize("ringtype", ["standard", "ConjugateInvariant"])
@pytest.mark.parametrize("level,B", SHAPES)
def test_mul_relin_then_rescale(torch_cuda, oracle_mod, monkeypatch, level, B, ringtype):
    """MulRelinCiphertextNew -> Rescale in place, with the same three checks
    (the oracle on the Standard ring)."""
    rng = np.random.default_rng(200 * level + B)
    res = {}
    x = None
    for defer in (False, True):
        lib = scheme(monkeypatch, defer, ringtype=ringtype)
        mods = lib.moduli()
        if x is None:
            x = plant_runs(rand_ct(rng, mods, level, lib.N, B=B), mods)
        ct = lib.import_ciphertext(x, 2.0 ** 40)
        lib.Rescale(lib.MulRelinCiphertextNew(ct, ct))  # (tables: first use)

        def run():
            cc = lib.MulRelinCiphertextNew(ct, ct)
            assert lib.Rescale(cc) == cc
            return cc

        cc, prof = profiled(lib, run)
        assert lib.GetCiphertextLevel(cc) == level - 1
        got = lib.export_ciphertext(cc)
        res[defer] = (got, prof)
        if defer and ringtype == "standard":
            orc = oracle_mod.Oracle(SMALL["logn"], mods, len(SMALL["logq"]), len(SMALL["logp"]))
            rlk = lib.export_relin_key()
            for b in (0, B - 1):
                ref = orc.rescale(orc.mul_relin(x[b], x[b], rlk, level), level)
                assert np.array_equal(got[b], ref), b
        lib.DeleteScheme()
    assert np.array_equal(res[True][0], res[False][0])
    assert_merged(res[True][1], res[False][1])


def test_every_exit_from_the_deferral(torch_cuda, monkeypatch):
    """Whatever follows the call that left its ModDown pending, the handles
    hold what the op-by-op calls give: the pending handle exported before the
    rescale; AddPlaintext on it first; rescaled from a second thread (the same
    context) and, with thread pipelines, read from another context before its
    own thread rescales it; deleted unread (no launch, no handle left); and a
    level-0 product, whose Rescale fails with the op-by-op message and which
    still reads back the plain ModDown's result."""
    level, B = 3, 8
    rng = np.random.default_rng(31)
    vals = rng.standard_normal((1 << SMALL["logn"]) // 2).astype(np.float32)

    # op by op
    lib = scheme(monkeypatch, False)
    mods = lib.moduli()
    x = plant_runs(rand_ct(rng, mods, level, lib.N, B=B), mods)
    ct = lib.import_ciphertext(x, 2.0 ** 20)
    cc = lib.MulRelinCiphertextNew(ct, ct)
    ref_md = lib.export_ciphertext(cc)
    ca = lib.CloneCiphertext(cc)
    lib.AddPlaintext(ca, lib.Encode(list(vals), level, 1 << 40))
    lib.Rescale(ca)
    ref_add = lib.export_ciphertext(ca)
    lib.Rescale(cc)
    ref_rs = lib.export_ciphertext(cc)
    c0 = lib.import_ciphertext(x[:, :, :1], 2.0 ** 20)
    ref_l0 = lib.export_ciphertext(lib.MulRelinCiphertextNew(c0, c0))
    lib.DeleteScheme()

    lib = scheme(monkeypatch, True)
    assert lib.moduli() == mods
    ct = lib.import_ciphertext(x, 2.0 ** 20)
    pt = lib.Encode(list(vals), level, 1 << 40)
    lib.Rescale(lib.MulRelinCiphertextNew(ct, ct))  # (tables: first use)
    # 1. exported before the rescale: the plain ModDown runs, then the plain rescale
    cc = lib.MulRelinCiphertextNew(ct, ct)
    assert lib.GetCiphertextLevel(cc) == level and lib.GetCiphertextBatch(cc) == B  # (metadata: still pending)
    assert np.array_equal(lib.export_ciphertext(cc), ref_md)
    _, pp = profiled(lib, lambda: lib.Rescale(cc))
    assert np.array_equal(lib.export_ciphertext(cc), ref_rs)
    lib.DeleteCiphertext(cc)
    # 2. AddPlaintext first
    cc = lib.MulRelinCiphertextNew(ct, ct)
    lib.AddPlaintext(cc, pt)
    lib.Rescale(cc)
    assert np.array_equal(lib.export_ciphertext(cc), ref_add)
    lib.DeleteCiphertext(cc)
    # 3a. rescaled by a second thread: the same context, the merged route
    cc = lib.MulRelinCiphertextNew(ct, ct)
    err = []

    def other():
        try:
            lib.Rescale(cc)
        except BaseException as e:  # reported below
            err.append(e)

    def threaded():
        t = threading.Thread(target=other)
        t.start()
        t.join()

    _, pt3 = profiled(lib, threaded)
    assert not err, err
    assert np.array_equal(lib.export_ciphertext(cc), ref_rs)
    assert (pt3["ntt_inv"], pt3["basis_ext"], pt3["ntt_fwd"]) == (1, 1, 1), pt3  # the three merged launches
    lib.DeleteCiphertext(cc)
    # 4. deleted unread: nothing runs, no handle stays
    live = sorted(lib.GetLiveCiphertexts())
    cc = lib.MulRelinCiphertextNew(ct, ct)
    assert sorted(lib.GetLiveCiphertexts()) == sorted(live + [cc])
    _, pd = profiled(lib, lambda: lib.DeleteCiphertext(cc))
    assert all(v == 0 for v in pd.values()), pd
    assert sorted(lib.GetLiveCiphertexts()) == live
    assert np.array_equal(lib.export_ciphertext(ct), x)
    # 5. level 0: today's error, the plain ModDown's result
    c0 = lib.import_ciphertext(x[:, :, :1], 2.0 ** 20)
    p0 = lib.MulRelinCiphertextNew(c0, c0)
    with pytest.raises(RuntimeError, match="cannot rescale a level-0 ciphertext"):
        lib.Rescale(p0)
    assert lib.GetCiphertextLevel(p0) == 0
    assert np.array_equal(lib.export_ciphertext(p0), ref_l0)
    # 3b. another context reads the pending handle of a pipeline's thread
    from orion_amd.replay import Pipelines
    pipes = Pipelines(lib, 1, device=0)
    try:
        ctp = pipes.run_one(0, lambda: lib.import_ciphertext(x, 2.0 ** 20))
        pipes.run_one(0, lambda: lib.Rescale(lib.MulRelinCiphertextNew(ctp, ctp)))  # (the pipeline's tables)
        cp = pipes.run_one(0, lambda: lib.MulRelinCiphertextNew(ctp, ctp))
        assert cp >> 20 == pipes.contexts[0]
        assert np.array_equal(lib.export_ciphertext(cp), ref_md)  # read from the scheme's thread
        with pytest.raises(RuntimeError, match="only by the context"):
            lib.Rescale(cp)  # an in-place op from another context is refused, as ever
        pipes.run_one(0, lambda: lib.Rescale(cp))
        assert np.array_equal(lib.export_ciphertext(cp), ref_rs)
        # ... and left alone, the pipeline's own thread takes the merged route
        cp2 = pipes.run_one(0, lambda: lib.MulRelinCiphertextNew(ctp, ctp))
        pipes.run_one(0, lambda: lib.Rescale(cp2))
        assert np.array_equal(lib.export_ciphertext(cp2), ref_rs)
    finally:
        pipes.close()
    # (the rescale after the export in 1. was the plain one: no basis extension in it)
    assert (pp["ntt_inv"], pp["basis_ext"], pp["ntt_fwd"]) == (1, 0, 1), pp
    lib.DeleteScheme()


def test_small_launch_keeps_the_latency_path(torch_cuda, monkeypatch):
    """B = 1 at N = 2^15: the ModDown's 2 (level + 1) limb-transforms take the
    fused latency path (the extension in the NTT's prologue), which has no
    merged form: same result, same launches as with the deferral off."""
    logq, logp = [60, 40, 40, 40, 40, 40], [60, 60]
    level = len(logq) - 1
    rng = np.random.default_rng(41)
    res = {}
    x = None
    for defer in (False, True):
        lib = scheme(monkeypatch, defer, logn=15, logq=logq, logp=logp)
        mods = lib.moduli()
        if x is None:
            x = plant_runs(rand_ct(rng, mods, level, lib.N, B=1), mods)
        ct = lib.import_ciphertext(x, 2.0 ** 40)
        lib.Rescale(lib.MulRelinCiphertextNew(ct, ct))
        cc, prof = profiled(lib, lambda: lib.Rescale(lib.MulRelinCiphertextNew(ct, ct)))
        res[defer] = (lib.export_ciphertext(cc), prof)
        lib.DeleteScheme()
    assert np.array_equal(res[True][0], res[False][0])
    assert res[True][1] == res[False][1], res
    assert res[True][1]["basis_ext"] == 0 and res[True][1]["ntt_bext"] > 0, res[True][1]


@pytest.mark.parametrize("K", [4, 8])
def test_source_counts_4_and_8(torch_cuda, monkeypatch, K):
    """basis_ext_rescale_kernel<4> and <8>: four and eight 61-bit P primes over
    a [60] + [30] x 8 chain (wide sources onto 30-bit targets and the 60-bit
    q_0; 30-bit pivots): three mul_relin -> rescale steps from the top and
    one at level 1 (a single output limb), merged against op by op."""
    logq, logp = [60] + [30] * 8, [61] * K
    top = len(logq) - 1
    rng = np.random.default_rng(50 + K)
    res = {}
    x = None
    for defer in (False, True):
        lib = scheme(monkeypatch, defer, logq=logq, logp=logp)
        mods = lib.moduli()
        if x is None:
            x = plant_runs(rand_ct(rng, mods, top, lib.N, B=2), mods)
        outs, profs = [], []
        ct = lib.import_ciphertext(x, 2.0 ** 30)
        for step in range(3):
            lib.Rescale(lib.MulRelinCiphertextNew(ct, ct))  # (tables: first use)
            nxt, p = profiled(lib, lambda: lib.Rescale(lib.MulRelinCiphertextNew(ct, ct)))
            outs.append(lib.export_ciphertext(nxt))
            profs.append(p)
            ct = nxt
        c1 = lib.import_ciphertext(x[:, :, :2], 2.0 ** 30)
        lib.Rescale(lib.MulRelinCiphertextNew(c1, c1))
        nxt, p = profiled(lib, lambda: lib.Rescale(lib.MulRelinCiphertextNew(c1, c1)))
        outs.append(lib.export_ciphertext(nxt))
        profs.append(p)
        res[defer] = (outs, profs)
        lib.DeleteScheme()
    for i, (a, b) in enumerate(zip(res[True][0], res[False][0])):
        assert np.array_equal(a, b), i
    for pm, pu in zip(res[True][1], res[False][1]):
        assert_merged(pm, pu)
