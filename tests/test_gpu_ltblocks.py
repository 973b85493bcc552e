"""GPU tests of the blocked linear transform (OrionHipNewLinearTransformBlocks /
OrionHipEvaluateLinearTransformBlocks): an R x C matrix of BSGS transforms as
one call, hoisted across rows and columns.

The reference is a restatement of the call's definition (include/orion_hip.h)
from the oracle's primitives -- gadget product, automorphism, coefficient
product, ModDown, rescale -- and numpy modular additions, fed with the
library's exported diagonals and Galois keys; with one column each row must
also be bit-equal to its own EvaluateLinearTransform (the 1 x 1 block: the
same code, so those tests hold both sides against the restatement too)."""
import numpy as np
import pytest

from tests.helpers import SMALL, SchemeCache, bsgs_split, plant_runs, rand_ct

pytestmark = pytest.mark.gpu

SCALE = float(2 ** 40)
BIG = [0, 1, 2, 3, 17, 64, 65, 300, 4095]
IDX_2X3 = [[BIG, [0], [5, 64, 128, 192]],
           [[1, 2, 3], [64, 128, 4000], BIG]]
N1_2X3 = [[32, 1, 128], [2, 256, 32]]
BAND = list(range(768))
# one baby (amount 0) and 66 giants, 65 of them rotating: N1 = 1 at any ratio
MANY_GIANTS = list(range(65)) + [2048]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_cache = SchemeCache()


# A baby-step / giant-step ratio of at most 2, i.e. Lattigo's
# LogBabyStepGiantStepRatio = 1: GenerateLinearTransform takes the natural
# logarithm of its argument and truncates it (lineartransform.go:67), so the
# argument is 4.0 (int(ln 4) = 1; an argument of 2.0 would mean a ratio of 1).
# It is the ratio at which the index sets below split with N1_2X3 and the band
# with N1 = 32, by the rule of oracle_find_best_bsgs_n1.
BSGS_RATIO = 4.0


def _gen(lib, rng, idx, level, ratio=BSGS_RATIO):
    diags = rng.uniform(-1, 1, (len(idx), lib.slots)).astype(np.float32)
    return lib.GenerateLinearTransform(idx, list(diags.reshape(-1)), level, ratio, "none"), diags


@pytest.fixture
def env(torch_cuda, oracle_mod):
    """(lib, oracle, transforms): the SMALL chain with every transform of the
    module generated before the keys, so each key is made once, for the highest
    level that uses it."""

    def make():
        from orion_amd.backend import HipLibrary
        lib = HipLibrary().new_scheme(SMALL["logn"], SMALL["logq"], SMALL["logp"], 40, h=192, seed=77)
        orc = oracle_mod.Oracle(SMALL["logn"], lib.moduli(), len(SMALL["logq"]), len(SMALL["logp"]))
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        lib.GenerateRelinearizationKey()
        rng = np.random.default_rng(2301)
        lts = dict(
            m23=[[_gen(lib, rng, idx, 3) for idx in row] for row in IDX_2X3],
            band=[[_gen(lib, rng, BAND, 1)] for _ in range(3)],
            zero=[[_gen(lib, rng, [0], 3), _gen(lib, rng, [0], 3)]],
            other_level=_gen(lib, rng, [0, 1], 2),
            many_giants=_gen(lib, rng, MANY_GIANTS, 1, ratio=1e9),
        )
        every = [t for k in ("m23", "band", "zero") for row in lts[k] for t, _ in row]
        every += [lts["other_level"][0], lts["many_giants"][0]]
        gels = sorted({g for t in every for g in lib.GetLinearTransformRotationKeys(t)})
        lib.GenerateConsolidatedRotationKeys(gels)
        return lib, orc, lts

    return _cache.get(make)


def _ids(rows):
    return [[t for t, _ in row] for row in rows]


# ---- the definition, restated --------------------------------------------------
def _addmod(a, b, q):
    s = a + b  # q < 2^61: no wrap
    return np.where(s >= q, s - q, s)


class Restated:
    def __init__(self, lib, orc, level):
        self.lib, self.orc, self.level = lib, orc, level
        mods = lib.moduli()
        self.qp = orc.qp_mods(level)
        self.q = np.array([mods[m] for m in self.qp], dtype=np.uint64)[:, None]
        P = 1
        for k in range(lib.K):
            P *= mods[lib.L + k]
        self.pq = np.zeros((level + 1, lib.N), dtype=np.uint64)
        for j in range(level + 1):
            self.pq[j, :] = P % mods[j]
        self.keys = {}

    def key(self, amount):
        g = int(self.lib.GaloisElement(amount))
        if g not in self.keys:
            self.keys[g] = self.lib.export_galois_key(g)
        return g, self.keys[g]

    def add(self, a, b):
        return _addmod(a, b, self.q)

    def mul(self, a, b):
        return self.orc.mul_coeffs(a, b, self.qp)

    def baby(self, x, b):
        """rot_b of one image x [2][level+1][N]: (c0, c1), each [nqp][N]"""
        nq, orc = self.level + 1, self.orc
        pc0 = orc.mul_coeffs(x[0, :nq], self.pq, list(range(nq)))
        zeros = np.zeros((self.lib.K, self.lib.N), dtype=np.uint64)
        if b == 0:
            pc1 = orc.mul_coeffs(x[1, :nq], self.pq, list(range(nq)))
            return np.concatenate([pc0, zeros]), np.concatenate([pc1, zeros])
        g, key = self.key(b)
        u0, u1 = orc.gadget_product_lazy(x[1, :nq], key, self.level)
        u0 = self.add(u0, np.concatenate([pc0, zeros]))
        return orc.automorphism_ntt(u0, g), orc.automorphism_ntt(u1, g)

    def blocks(self, xs, members, rescale):
        """xs[j]: image of column j; members[i][j] = (transform handle, index
        list, N1).  Returns out[i] [2][level(+1)][N]."""
        lib, orc, level = self.lib, self.orc, self.level
        nqp = level + 1 + lib.K
        C = len(xs)
        rots = [dict() for _ in range(C)]
        out = []
        for row in members:
            t = {}  # giant amount -> [c0, c1]
            for j, (lt, idx, n1) in enumerate(row):
                for d in idx:
                    g, b = bsgs_split(d, lib.slots, n1)
                    if b not in rots[j]:
                        rots[j][b] = self.baby(xs[j], b)
                    pt = lib.export_lt_diagonal(lt, d, level)
                    cur = t.setdefault(g, [np.zeros((nqp, lib.N), dtype=np.uint64) for _ in range(2)])
                    for c in range(2):
                        cur[c] = self.add(cur[c], self.mul(pt, rots[j][b][c]))
            acc = [np.zeros((nqp, lib.N), dtype=np.uint64) for _ in range(2)]
            for g, (t0, t1) in t.items():
                if g != 0:
                    gel, key = self.key(g)
                    c0, c1 = orc.gadget_product_lazy(orc.moddown(t1, level), key, level)
                    c0 = self.add(c0, t0)
                    t0, t1 = orc.automorphism_ntt(c0, gel), orc.automorphism_ntt(c1, gel)
                acc = [self.add(acc[0], t0), self.add(acc[1], t1)]
            y = np.stack([orc.moddown(acc[0], level), orc.moddown(acc[1], level)])
            out.append(orc.rescale(y, level) if rescale else y)
        return out


def _members(rows, idxs, lib):
    return [[(t, idx, lib.GetLinearTransformN1(t)) for (t, _), idx in zip(row, irow)] for row, irow in zip(rows, idxs)]


def _planted(lib, level, B, seed):
    mods = lib.moduli()
    return plant_runs(rand_ct(np.random.default_rng(seed), mods, level, lib.N, B=B), mods)


def _delete(lib, cts):
    for c in cts:
        lib.DeleteCiphertext(c)


# ---- 1. oracle parity ---------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0, 1])
def test_2x3_matches_the_definition(env, rescale):
    lib, orc, lts = env
    rows = lts["m23"]
    assert [[lib.GetLinearTransformN1(t) for t, _ in row] for row in rows] == N1_2X3
    assert [[orc.find_best_bsgs_n1(idx, 1) for idx in row] for row in IDX_2X3] == N1_2X3
    B, level = 2, 3
    xs = [_planted(lib, level, B, 10 + j) for j in range(3)]
    cts = [lib.import_ciphertext(x, SCALE) for x in xs]
    blk = lib.new_linear_transform_blocks(_ids(rows))
    outs = lib.evaluate_linear_transform_blocks(blk, cts, rescale=rescale)
    assert len(outs) == 2
    got = [lib.export_ciphertext(o) for o in outs]
    ref = Restated(lib, orc, level)
    mem = _members(rows, IDX_2X3, lib)
    q3 = lib.moduli()[3]
    for b in (0, B - 1):
        exp = ref.blocks([x[b] for x in xs], mem, rescale)
        for i in range(2):
            assert got[i].shape[0] == B and lib.GetCiphertextLevel(outs[i]) == level - rescale
            assert np.array_equal(got[i][b], exp[i]), (b, i)
    for o in outs:
        assert lib.GetCiphertextScaleF(o) == (SCALE if rescale else SCALE * q3)
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, cts + outs)


# ---- 2. the existing path ------------------------------------------------------------
def test_1x1_is_evaluate_linear_transform(env):
    lib, orc, lts = env
    t = lts["m23"][0][0][0]
    x = _planted(lib, 3, 2, 20)
    ct = lib.import_ciphertext(x, SCALE)
    blk = lib.new_linear_transform_blocks([[t]])
    ref = Restated(lib, orc, 3)
    mem = [[(t, BIG, lib.GetLinearTransformN1(t))]]
    for rescale in (0, 1):
        one = lib.EvaluateLinearTransform(t, ct)
        if rescale:
            lib.Rescale(one)
        (out,) = lib.evaluate_linear_transform_blocks(blk, [ct], rescale=rescale)
        got = lib.export_ciphertext(one)
        assert np.array_equal(lib.export_ciphertext(out), got), rescale
        assert lib.GetCiphertextScaleF(out) == lib.GetCiphertextScaleF(one)
        for b in (0, 1):  # (both calls run the same code: the restatement is the witness)
            (exp,) = ref.blocks([x[b]], mem, rescale)
            assert np.array_equal(got[b], exp), (rescale, b)
        _delete(lib, [one, out])
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, [ct])


def test_3x1_band_two_baby_passes_two_chunks(env):
    """Three blocks of the dense band range(768): N1 = 32, 24 giants and 32
    babies each -- two passes of 16 register slots, 72 (row, giant) entries in
    two plan chunks of 64; one column, so each row is its own transform.  Row 0
    is also held against the restatement (a single transform is the 1 x 1 block:
    both calls run the same code; its 768 diagonals cost the restatement about
    1.3 s of CPU)."""
    lib, orc, lts = env
    rows = lts["band"]
    assert all(lib.GetLinearTransformN1(t) == 32 for (t, _), in rows)
    x = _planted(lib, 1, 1, 21)
    ct = lib.import_ciphertext(x, SCALE)
    blk = lib.new_linear_transform_blocks(_ids(rows))
    outs = lib.evaluate_linear_transform_blocks(blk, [ct], rescale=0)
    (exp,) = Restated(lib, orc, 1).blocks([x[0]], [[(rows[0][0][0], BAND, 32)]], 0)
    assert np.array_equal(lib.export_ciphertext(outs[0])[0], exp)
    for i, ((t, _),) in enumerate(rows):
        one = lib.EvaluateLinearTransform(t, ct)
        assert np.array_equal(lib.export_ciphertext(outs[i]), lib.export_ciphertext(one)), i
        _delete(lib, [one])
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, [ct] + outs)


def test_single_transform_with_two_plan_chunks(env):
    """One baby (amount 0) and 66 giants, 65 of them rotating -- more than the
    64 entries of a plan chunk and the 64 giants of a giant-phase launch: two
    plan chunks in the baby phase, partial sums in the giant phase.  (The
    restatement: about 0.3 s of CPU.)"""
    lib, orc, lts = env
    t, _ = lts["many_giants"]
    # (GenerateLinearTransform truncates ln(1e9) to 20; the ratio never reaches 2^20)
    assert lib.GetLinearTransformN1(t) == 1 == orc.find_best_bsgs_n1(MANY_GIANTS, 20)
    x = _planted(lib, 1, 1, 22)
    ct = lib.import_ciphertext(x, SCALE)
    one = lib.EvaluateLinearTransform(t, ct)
    (exp,) = Restated(lib, orc, 1).blocks([x[0]], [[(t, MANY_GIANTS, 1)]], 0)
    assert np.array_equal(lib.export_ciphertext(one)[0], exp)
    _delete(lib, [ct, one])


def test_1x2_without_a_rotating_giant(env):
    lib, orc, lts = env
    rows = lts["zero"]
    xs = [_planted(lib, 3, 2, 30 + j) for j in range(2)]
    cts = [lib.import_ciphertext(x, SCALE) for x in xs]
    blk = lib.new_linear_transform_blocks(_ids(rows))
    (out,) = lib.evaluate_linear_transform_blocks(blk, cts, rescale=1)
    got = lib.export_ciphertext(out)
    ref = Restated(lib, orc, 3)
    for b in (0, 1):
        (exp,) = ref.blocks([x[b] for x in xs], _members(rows, [[[0], [0]]], lib), 1)
        assert np.array_equal(got[b], exp), b
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, cts + [out])


def test_conjugate_invariant_2x1(torch_cuda):
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(SMALL["logn"], SMALL["logq"], SMALL["logp"], 40, h=192, seed=78,
                                  ringtype="ConjugateInvariant")
    try:
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        rng = np.random.default_rng(2302)
        ts = [_gen(lib, rng, idx, 3)[0] for idx in ([0, 1, 2, 3, 17, 64, 65, 300], [5, 64, 128, 192])]
        lib.GenerateConsolidatedRotationKeys(sorted({g for t in ts for g in lib.GetLinearTransformRotationKeys(t)}))
        ct = lib.import_ciphertext(_planted(lib, 3, 2, 40), SCALE)
        blk = lib.new_linear_transform_blocks([[ts[0]], [ts[1]]])
        outs = lib.evaluate_linear_transform_blocks(blk, [ct], rescale=1)
        for t, o in zip(ts, outs):
            one = lib.EvaluateLinearTransform(t, ct)
            lib.Rescale(one)
            assert np.array_equal(lib.export_ciphertext(o), lib.export_ciphertext(one))
    finally:
        lib.DeleteScheme()


# ---- 3. functional ---------------------------------------------------------------------
def test_2x3_decrypts_to_the_matrix_product(env):
    lib, orc, lts = env
    rows = lts["m23"]
    rng = np.random.default_rng(50)
    vals = rng.standard_normal((3, lib.slots)).astype(np.float32)
    cts = [lib.Encrypt(lib.Encode(list(v), 3, 1 << 40)) for v in vals]
    blk = lib.new_linear_transform_blocks(_ids(rows))
    outs = lib.evaluate_linear_transform_blocks(blk, cts, rescale=1)
    worst = 0.0
    for i, o in enumerate(outs):
        exp = sum(diags[k].astype(np.float64) * np.roll(vals[j].astype(np.float64), -d)
                  for j, ((_, diags), idx) in enumerate(zip(rows[i], IDX_2X3[i])) for k, d in enumerate(idx))
        dec = np.array(lib.Decode(lib.Decrypt(o)))
        worst = max(worst, float(np.abs(dec - exp).max()))
    print("2x3 blocked, max |decoded - expected| =", worst)
    assert worst < 3 * 1e-3  # the single-transform bound (test_gpu_parity.py), once per column
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, cts + outs)


# ---- 4. launch counts ------------------------------------------------------------------
def _profiled(lib, fn):
    lib.OrionHipSynchronize()
    lib.OrionHipProfileReset()
    lib.OrionHipProfile(1)
    made = fn()
    lib.OrionHipSynchronize()
    lib.OrionHipProfile(0)
    return lib.profile_read(), made


def _loop(lib, rows, cts):
    """the frontend's loop (lt_evaluator.py): per row, transforms added across the columns, one rescale"""
    outs = []
    for row in rows:
        acc = None
        for (t, _), c in zip(row, cts):
            y = lib.EvaluateLinearTransform(t, c)
            if acc is None:
                acc = y
            else:
                s = lib.AddCiphertextNew(acc, y)
                _delete(lib, [acc, y])
                acc = s
        outs.append(lib.RescaleNew(acc))
        _delete(lib, [acc])
    return outs


def test_launch_counts_against_the_loop(env):
    lib, orc, lts = env
    rows = lts["m23"]
    cts = [lib.import_ciphertext(_planted(lib, 3, 2, 60 + j), SCALE) for j in range(3)]
    blk = lib.new_linear_transform_blocks(_ids(rows))
    _delete(lib, lib.evaluate_linear_transform_blocks(blk, cts) + _loop(lib, rows, cts))  # warm
    pl, lo = _profiled(lib, lambda: _loop(lib, rows, cts))
    pb, bo = _profiled(lib, lambda: lib.evaluate_linear_transform_blocks(blk, cts))
    n = lambda p, k: p.get(k, {}).get("launches", 0)  # noqa: E731
    print("category           loop  blocked")
    for k in sorted(set(pl) | set(pb)):
        print(f"{k:18s} {n(pl, k):5d} {n(pb, k):7d}")
    R, C = 2, 3
    # (the block with no rotation has no giant phase of its own in the loop)
    assert n(pl, "lt_giant") == R * C - 1 and 1 <= n(pb, "lt_giant") <= R
    # no launch for the additions: the blocked call's only elementwise launches cut the R rows from the batch
    assert n(pb, "elementwise") <= R and n(pl, "elementwise") >= R * (C - 1)
    assert n(pb, "ntt_inv") < n(pl, "ntt_inv") and n(pb, "ntt_fwd") < n(pl, "ntt_fwd")
    assert n(pb, "basis_ext") + n(pb, "ntt_bext") < n(pl, "basis_ext") + n(pl, "ntt_bext")
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, cts + lo + bo)


# ---- 5. contracts ------------------------------------------------------------------------
def test_errors_leave_the_handles_alone(env):
    lib, orc, lts = env
    rows = lts["m23"]
    ids = _ids(rows)
    x = _planted(lib, 3, 2, 70)
    cts = [lib.import_ciphertext(x, SCALE) for _ in range(3)]
    lo = lib.import_ciphertext(x[:, :, :3], SCALE)
    one = lib.import_ciphertext(x[:1], SCALE)
    scaled = lib.import_ciphertext(x, SCALE)
    lib.SetCiphertextScale(scaled, 2 ** 41)
    l0 = lib.import_ciphertext(x[:, :, :1], SCALE)
    blk = lib.new_linear_transform_blocks(ids)
    live = sorted(lib.GetLiveCiphertexts())
    live_pts = sorted(lib.GetLivePlaintexts())
    unknown = max(live) + 1000
    other = lts["other_level"][0]

    def refused(match, fn, *args, **kw):
        with pytest.raises(RuntimeError, match=match):
            fn(*args, **kw)
        assert sorted(lib.GetLiveCiphertexts()) == live and sorted(lib.GetLivePlaintexts()) == live_pts, match

    from orion_amd.backend import c_int
    three = (c_int * 3)(*cts)
    two = (c_int * 2)()
    assert lib.lib.OrionHipNewLinearTransformBlocks(None, 1, 1) == -1 and b"null" in lib.lib.OrionHipLastError()
    assert lib.lib.OrionHipEvaluateLinearTransformBlocks(blk, None, 0, two) == -1
    assert lib.lib.OrionHipEvaluateLinearTransformBlocks(blk, three, 0, None) == -1
    assert lib.lib.OrionHipNewLinearTransformBlocks((c_int * 1)(ids[0][0]), 0, 1) == -1
    assert b"at least one row" in lib.lib.OrionHipLastError()
    assert lib.lib.OrionHipNewLinearTransformBlocks((c_int * 1)(ids[0][0]), 1, 0) == -1
    assert sorted(lib.GetLiveCiphertexts()) == live
    refused("handle not found: 999999", lib.new_linear_transform_blocks, [[ids[0][0], 999999]])
    refused(rf"{ids[0][0]} \(level 3\) and {other} \(level 2\): the levels differ",
            lib.new_linear_transform_blocks, [[ids[0][0], other]])
    refused(f"handle not found: {unknown}", lib.evaluate_linear_transform_blocks, blk, [cts[0], unknown, cts[2]])
    refused(rf"{cts[0]} \(level 3\) and {lo} \(level 2\): the levels differ",
            lib.evaluate_linear_transform_blocks, blk, [cts[0], cts[1], lo])
    refused(rf"{cts[0]} \(scale 1099511627776\) and {scaled} \(scale 2199023255552\): the scales differ",
            lib.evaluate_linear_transform_blocks, blk, [cts[0], scaled, cts[2]])
    refused(rf"{cts[0]} \(batch 2\) and {one} \(batch 1\): the batches differ",
            lib.evaluate_linear_transform_blocks, blk, [cts[0], cts[1], one])
    refused("level-0", lib.evaluate_linear_transform_blocks, blk, [l0, l0, l0], rescale=True)
    refused("handle not found", lib.evaluate_linear_transform_blocks, blk + 1000, cts)
    # a column whose blocks need more than 64 distinct baby rotations between them: N1 = 64 with babies
    # 0..40 (21 giants: ratio 40 / 20) over N1 = 128 with babies 64..103 and 0 (21 giants): 81 amounts
    rng = np.random.default_rng(71)
    wide = [_gen(lib, rng, list(range(41)) + [64 * k for k in range(1, 21)], 3)[0],
            _gen(lib, rng, list(range(64, 104)) + [128 * k for k in range(1, 21)], 3)[0]]
    assert [lib.GetLinearTransformN1(t) for t in wide] == [64, 128]
    refused("column 0 .* 81 baby steps: more than 64", lib.new_linear_transform_blocks, [[wide[0]], [wide[1]]])
    lonely = _gen(lib, rng, [0, 777], 3)[0]
    b2 = lib.new_linear_transform_blocks([[lonely]])
    # a member whose diagonals are gone
    lib.RemovePlaintextDiagonals(lonely)
    refused("not loaded", lib.evaluate_linear_transform_blocks, b2, [cts[0]])
    refused("not loaded", lib.new_linear_transform_blocks, [[lonely]])
    # a deleted member is named, and a new transform on its handle id is not mistaken for it
    lib.DeleteLinearTransform(lonely)
    refused(f"member transform {lonely} has been deleted", lib.evaluate_linear_transform_blocks, b2, [cts[0]])
    again = _gen(lib, rng, [0], 3)[0]
    assert again == lonely  # lowest free id
    refused(f"member transform {lonely} has been deleted", lib.evaluate_linear_transform_blocks, b2, [cts[0]])
    # the first blocks object still works
    outs = lib.evaluate_linear_transform_blocks(blk, cts)
    assert len(outs) == 2
    for t in wide + [again]:
        lib.DeleteLinearTransform(t)
    lib.delete_linear_transform_blocks(b2)
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, cts + [lo, one, scaled, l0] + outs)


def test_poisoned_source_is_refused(torch_cuda):
    """One column of the 2 x 3 call is a ciphertext whose deferred rotate-and-add
    failed (an allocation past the pool cap, the recipe of
    test_deferred_rotation_failure_poisons; a scheme of its own, whose pool has
    cached nothing the key switch could reuse): the call reports the poison,
    allocates no row and leaves the handle lists alone."""
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(SMALL["logn"], SMALL["logq"], SMALL["logp"], 40, h=192, seed=80)
    try:
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        rng = np.random.default_rng(2304)
        ids = [[_gen(lib, rng, idx, 3)[0] for idx in row] for row in IDX_2X3]
        lib.GenerateConsolidatedRotationKeys(
            sorted({g for row in ids for t in row for g in lib.GetLinearTransformRotationKeys(t)}))
        blk = lib.new_linear_transform_blocks(ids)
        cts = [lib.import_ciphertext(_planted(lib, 5, 2, 100 + j), SCALE) for j in range(3)]
        x = cts[1]
        r = lib.RotateNew(x, 1)  # (rotation 1 is a baby step of BIG: its key exists)
        assert lib.AddCiphertext(x, r) == x
        st = lib.pool_stats()
        lib.pool_cap(st["held_bytes"] - st["cached_bytes"])  # nothing new fits
        try:
            with pytest.raises(RuntimeError, match="device memory exhausted"):
                lib.DeleteCiphertext(r)
        finally:
            lib.pool_cap(0)
        live, live_pts = sorted(lib.GetLiveCiphertexts()), sorted(lib.GetLivePlaintexts())
        assert r not in live and x in live
        with pytest.raises(RuntimeError, match="deferred rotation by 1 failed"):
            lib.evaluate_linear_transform_blocks(blk, cts)
        assert sorted(lib.GetLiveCiphertexts()) == live and sorted(lib.GetLivePlaintexts()) == live_pts
        # with a sound ciphertext in its place the same call goes through
        cts[1] = lib.import_ciphertext(_planted(lib, 5, 2, 101), SCALE)
        outs = lib.evaluate_linear_transform_blocks(blk, cts)
        assert len(outs) == 2 and all(lib.GetCiphertextLevel(o) == 2 for o in outs)
    finally:
        lib.DeleteScheme()


def test_missing_galois_key_without_the_secret_key(torch_cuda):
    """A scheme that never had the secret key (a server) cannot make the keys a
    layer needs on first use: the call fails with the key lookup's message
    before anything is queued, and allocates nothing."""
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(SMALL["logn"], SMALL["logq"], SMALL["logp"], 40, h=192, seed=79)
    try:
        rng = np.random.default_rng(2303)
        ts = [_gen(lib, rng, idx, 3)[0] for idx in ([0, 1, 2, 3], [0, 64])]
        cts = [lib.import_ciphertext(_planted(lib, 3, 1, 110 + j), SCALE) for j in range(2)]
        blk = lib.new_linear_transform_blocks([ts])  # 1 x 2: needs no key yet
        live = sorted(lib.GetLiveCiphertexts())
        with pytest.raises(RuntimeError, match="secret key not generated"):
            lib.evaluate_linear_transform_blocks(blk, cts)
        assert sorted(lib.GetLiveCiphertexts()) == live and lib.GetLivePlaintexts() == []
        with pytest.raises(RuntimeError, match="secret key not generated"):  # the members' own message
            lib.EvaluateLinearTransform(ts[0], cts[0])
    finally:
        lib.DeleteScheme()


def test_changed_member_rebuilds_the_plan(env):
    lib, orc, lts = env
    rng = np.random.default_rng(72)
    t, _ = _gen(lib, rng, [0, 1, 2, 3], 3)
    ct = lib.import_ciphertext(_planted(lib, 3, 1, 73), SCALE)
    blk = lib.new_linear_transform_blocks([[t]])
    (a,) = lib.evaluate_linear_transform_blocks(blk, [ct], rescale=0)
    blobs = {d: lib.SerializeDiagonal(t, d)[0] for d in (0, 1, 2, 3)}
    lib.RemovePlaintextDiagonals(t)
    for d in (0, 1, 2, 3):  # the same diagonals, rotated: 0 <- 1 <- 2 <- 3 <- 0
        lib.LoadPlaintextDiagonal(blobs[(d + 1) % 4], t, d)
    (b,) = lib.evaluate_linear_transform_blocks(blk, [ct], rescale=0)
    one = lib.EvaluateLinearTransform(t, ct)
    assert np.array_equal(lib.export_ciphertext(b), lib.export_ciphertext(one))
    assert not np.array_equal(lib.export_ciphertext(b), lib.export_ciphertext(a))
    lib.delete_linear_transform_blocks(blk)
    lib.DeleteLinearTransform(t)
    _delete(lib, [ct, a, b, one])


def test_captured_call_replays_to_the_same_bits(env):
    lib, orc, lts = env
    rows = lts["m23"]
    cts = [lib.import_ciphertext(_planted(lib, 3, 2, 80 + j), SCALE) for j in range(3)]
    blk = lib.new_linear_transform_blocks(_ids(rows))
    warm = lib.evaluate_linear_transform_blocks(blk, cts)
    exp = [lib.export_ciphertext(o) for o in warm]
    lib.OrionHipGraphBegin()
    try:
        outs = lib.evaluate_linear_transform_blocks(blk, cts)
    finally:
        gid = lib.OrionHipGraphEnd()
    assert lib.OrionHipGraphLaunch(gid) == 0
    lib.OrionHipSynchronize()
    for o, e in zip(outs, exp):
        assert np.array_equal(lib.export_ciphertext(o), e)
    lib.OrionHipGraphDestroy(gid)
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, cts + warm + outs)


def test_pipeline_thread_gives_the_scheme_threads_bits(env):
    from orion_amd.replay import Pipelines
    lib, orc, lts = env
    rows = lts["m23"]
    xs = [_planted(lib, 3, 2, 90 + j) for j in range(3)]
    cts = [lib.import_ciphertext(x, SCALE) for x in xs]
    blk = lib.new_linear_transform_blocks(_ids(rows))
    mine = lib.evaluate_linear_transform_blocks(blk, cts)
    exp = [lib.export_ciphertext(o) for o in mine]
    pipes = Pipelines(lib, 1, device=0)
    try:
        def work():
            outs = lib.evaluate_linear_transform_blocks(blk, cts)  # the scheme's blocks and ciphertexts, read
            got = [lib.export_ciphertext(o) for o in outs]
            for o in outs:
                lib.DeleteCiphertext(o)
            return outs, got

        outs, got = pipes.run_one(0, work)
        assert all(o >> 20 == pipes.contexts[0] for o in outs)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)
    finally:
        pipes.close()
        lib.thread_pipelines(pipes.prev)
    lib.delete_linear_transform_blocks(blk)
    _delete(lib, cts + mine)


# ---- 6. replay -----------------------------------------------------------------------------
def test_resnet_first_4x4_layer_replayed_blocked(torch_cuda):
    """The recorded ResNet-20 stream at N = 2^13 up to the last rescale of its
    first 4 x 4 convolution (the whole pass holds 42 bootstraps): the 4 x 1 input
    layer and the 4 x 4 layer each run as one blocked call; the decoded output
    row agrees with the plain replay's."""
    from orion_amd.replay import OrionStream, block_groups
    st = OrionStream("resnet20_n13", seed=91)
    lib = st.lib
    try:
        first = min((g for g in block_groups(st._events) if (g["rows"], g["cols"]) == (4, 4)), key=lambda g: g["start"])
        stop = first["end"]
        # the prefix alone: its transforms and plaintexts, no bootstrapper
        used = {t for g in block_groups(st._events) if g["end"] <= stop for row in g["lts"] for t in row}
        late = {id(e) for e in [e for e in st._events if e["phase"] == "forward"][stop + 1:]}
        st._events = [e for e in st._events if id(e) not in late and not (
            e["phase"] == "compile" and (e["op"] == "NewBootstrapper" or
                                         (e["op"] == "GenerateLinearTransform" and e["ret"] not in used)))]
        st.keygen()
        st.compile(blocked=True)
        assert sorted(st.block_map) == [g["start"] for g in block_groups(st._events) if g["rows"] * g["cols"] > 1]
        assert first["start"] in st.block_map
        ct = st.encrypt_batch(st.reference_input())
        live = sorted(lib.GetLiveCiphertexts())
        for replaced in (first["start"], first["start"] + 1):  # a transform and an addition the call replaces
            with pytest.raises(ValueError, match="stop_after"):
                st.forward(ct, stop_after=replaced, blocked=True)
        plain = st.forward(lib.CloneCiphertext(ct), stop_after=stop)
        mid = sorted(lib.GetLiveCiphertexts())
        blocked = st.forward(lib.CloneCiphertext(ct), stop_after=stop, blocked=True)
        # handle bookkeeping: each pass leaves its input and its output, nothing else
        assert len(mid) - len(live) == len(lib.GetLiveCiphertexts()) - len(mid) == 2
        assert lib.GetCiphertextLevel(plain) == lib.GetCiphertextLevel(blocked)
        assert lib.GetCiphertextScaleF(plain) == lib.GetCiphertextScaleF(blocked)
        a, b = (lib.decode_f64(lib.Decrypt(h)) for h in (plain, blocked))
        print("resnet20_n13 first 4x4 layer, max |blocked - plain| =", float(np.abs(a - b).max()),
              " max |plain| =", float(np.abs(a).max()))
        assert np.abs(a - b).max() < 1e-3
        assert not np.array_equal(lib.export_ciphertext(plain), lib.export_ciphertext(blocked))  # another definition
    finally:
        lib.DeleteScheme()
