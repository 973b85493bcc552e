"""GPU tests of lt_bsgs's shared-diagonal mapping (csrc/kernels.hip,
lt_bsgs_body with IW = 4): launches of 4 images and more give a workgroup 64
coefficients of 4 images, and its waves load each diagonal row once between
them, through LDS.

Everything is bit-exact.  The first reference is the same call on one image
at a time: a one-image launch takes the one-image-per-workgroup kernel, whose
code the mapping leaves as it was.  The second, where the suite has it, is
the CPU oracle (its lt_bsgs, its replay of the recorded LoLA stream)."""
import numpy as np
import pytest

from tests.helpers import PLANT_CHAINS, SMALL, SchemeCache, bsgs_split, plant_runs, rand_ct

pytestmark = pytest.mark.gpu

SCALE = float(2 ** 40)
BSGS_RATIO = 4.0  # LogBabyStepGiantStepRatio = 1 (test_gpu_ltblocks.py)

# index sets by the (babies, giants) the BSGS rule gives them at 4096 slots;
# `pairs`: how many of the babies x giants diagonals exist
DENSE = list(range(48))  # N1 = 8: 8 x 6, all 48 pairs
SPARSE = [0, 1, 2, 3, 4, 5, 6, 7, 9, 19, 22, 24, 39, 42, 45]  # N1 = 8: 8 x 6, 15 pairs
BIG = [0, 1, 2, 3, 17, 64, 65, 300, 4095]  # N1 = 32: 7 x 4, 9 pairs
B12 = list(range(12)) + [32 * k + j for k in range(1, 7) for j in (0, 5)]  # N1 = 32: 12 x 7 (one 16-slot launch)
B20 = list(range(20)) + [32 * k + (3 * k) % 20 for k in range(1, 11)]  # N1 = 32: 20 x 11 (16 slots, then 4 added)
BAND = list(range(768))  # N1 = 32: 32 x 24 (16 slots, then 16 added)
SHAPES = {"dense": (DENSE, 8, 8, 6), "sparse": (SPARSE, 8, 8, 6), "big": (BIG, 32, 7, 4), "b12": (B12, 32, 12, 7),
          "b20": (B20, 32, 20, 11), "band": (BAND, 32, 32, 24)}
IDX_2X3 = [[BIG, [0], [5, 64, 128, 192]],
           [[1, 2, 3], [64, 128, 4000], BIG]]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_cache = SchemeCache()
_cache61 = SchemeCache()


def _gen(lib, rng, idx, level):
    diags = rng.uniform(-1, 1, (len(idx), lib.slots)).astype(np.float32)
    return lib.GenerateLinearTransform(idx, list(diags.reshape(-1)), level, BSGS_RATIO, "none")


def _scheme(chain, seed, make_lts):
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(chain["logn"], chain["logq"], chain["logp"], 40, h=192, seed=seed)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    lts = make_lts(lib, np.random.default_rng(seed))
    handles = [int(t) for v in lts.values() for t in np.ravel(v)]  # (a handle, or rows of handles)
    lib.GenerateConsolidatedRotationKeys(sorted({g for t in handles for g in lib.GetLinearTransformRotationKeys(t)}))
    return lib, lts


@pytest.fixture
def env(torch_cuda, oracle_mod):
    """(lib, oracle, transforms) on the SMALL chain: q0 of 55 bits and two P
    limbs of 60 (the 30-bit-piece integer products), the rest 40 bits (the
    float64 products).  Level 3 has all three kinds."""

    def make():
        def lts(lib, rng):
            out = {k: _gen(lib, rng, SHAPES[k][0], 1 if k == "band" else 3) for k in SHAPES}
            out["m23"] = [[_gen(lib, rng, idx, 3) for idx in row] for row in IDX_2X3]
            return out

        lib, made = _scheme(SMALL, 177, lts)
        orc = oracle_mod.Oracle(SMALL["logn"], lib.moduli(), len(SMALL["logq"]), len(SMALL["logp"]))
        return lib, orc, made

    return _cache.get(make)


def _planted(lib, level, B, seed):
    mods = lib.moduli()
    return plant_runs(rand_ct(np.random.default_rng(seed), mods, level, lib.N, B=B), mods)


def _delete(lib, cts):
    for c in cts:
        lib.DeleteCiphertext(c)


def _batch_and_alone(lib, t, x):
    """EvaluateLinearTransform(t) of the batch x [B][2][limbs][N] as one call,
    and of each of its images as a call of its own: ([B]..., [B]...)"""
    ct = lib.import_ciphertext(x, SCALE)
    out = lib.EvaluateLinearTransform(t, ct)
    got = lib.export_ciphertext(out)
    _delete(lib, [ct, out])
    alone = []
    for b in range(x.shape[0]):
        c1 = lib.import_ciphertext(x[b:b + 1], SCALE)
        o1 = lib.EvaluateLinearTransform(t, c1)
        alone.append(lib.export_ciphertext(o1)[0])
        _delete(lib, [c1, o1])
    return got, np.stack(alone)


def _shape_check(lib, orc, name, t):
    idx, n1, nb, ng = SHAPES[name]
    assert lib.GetLinearTransformN1(t) == n1 == orc.find_best_bsgs_n1(idx, 1)
    split = [bsgs_split(d, lib.slots, n1) for d in idx]
    assert len({b for _, b in split}) == nb and len({g for g, _ in split}) == ng


def _oracle_lt(lib, orc, t, idx, level, x1):
    pts = [lib.export_lt_diagonal(t, d, level) for d in idx]
    gels = [g for g in lib.GetLinearTransformRotationKeys(t) if g != 1]
    return orc.lt_bsgs(x1, level, idx, pts, lib.GetLinearTransformN1(t), {g: lib.export_galois_key(g) for g in gels})


# ---- 1. batch sizes -------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 5, 7, 8])
def test_batch_sizes_match_each_image_alone(env, B):
    """B = 4 and 8: full groups of four; B = 5 and 7: a last group with three
    waves and one wave past the batch.  Level 3: limb 0 and the P limbs take
    the 30-bit-piece path, limbs 1..3 the float64 path.  The first and the
    last image are also held against the CPU oracle."""
    lib, orc, lts = env
    t = lts["dense"]
    _shape_check(lib, orc, "dense", t)
    bits = [int(q).bit_length() for q in lib.moduli()]
    assert bits[0] > 48 and all(b <= 48 for b in bits[1:4]) and all(b > 48 for b in bits[lib.L:])
    x = _planted(lib, 3, B, 400 + B)
    got, alone = _batch_and_alone(lib, t, x)
    assert got.shape == alone.shape and got.shape[0] == B
    for b in range(B):
        assert np.array_equal(got[b], alone[b]), b
    for b in (0, B - 1):
        assert np.array_equal(got[b], _oracle_lt(lib, orc, t, DENSE, 3, x[b])), b


# ---- 2. more babies than one launch's register slots ---------------------------------
@pytest.mark.parametrize("name", ["b12", "b20", "band"])
def test_more_babies_than_eight(env, name):
    """12 babies: one launch of the 16-slot kernel.  20: 16 slots, then a second
    launch (s0 = 16) of the 8-slot kernel that adds its 4 babies' products to
    the first's sums.  32 (the band, level 1): two 16-slot launches, the
    second adding.  B = 6: a full group and a group of two."""
    lib, orc, lts = env
    t = lts[name]
    _shape_check(lib, orc, name, t)
    level = 1 if name == "band" else 3
    B = 6
    x = _planted(lib, level, B, 420)
    got, alone = _batch_and_alone(lib, t, x)
    for b in range(B):
        assert np.array_equal(got[b], alone[b]), b
    if name != "band":  # (768 diagonals: the one-image kernel is the witness, as in test_gpu_ltblocks.py)
        assert np.array_equal(got[B - 1], _oracle_lt(lib, orc, t, SHAPES[name][0], level, x[B - 1]))


# ---- 3. sparse diagonals -------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "big"])
def test_sparse_diagonals(env, name):
    """Most (giant, baby) pairs have no diagonal: their plan slots carry the
    zero diagonal and a cleared mask bit.  B = 5."""
    lib, orc, lts = env
    t = lts[name]
    _shape_check(lib, orc, name, t)
    idx, _, nb, ng = SHAPES[name]
    assert len(idx) < nb * ng // 2
    B = 5
    x = _planted(lib, 3, B, 430)
    got, alone = _batch_and_alone(lib, t, x)
    for b in range(B):
        assert np.array_equal(got[b], alone[b]), b
    for b in (0, B - 1):
        assert np.array_equal(got[b], _oracle_lt(lib, orc, t, idx, 3, x[b])), b


# ---- 4. blocked layer ------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0, 1])
def test_blocked_2x3_with_five_images_per_column(env, rescale):
    """colB = 5: every column's launch has a full group and a group of one
    image, and each entry's output row (row * 5 + image) comes from the plan."""
    lib, orc, lts = env
    ids = lts["m23"]
    B = 5
    xs = [_planted(lib, 3, B, 440 + j) for j in range(3)]
    cts = [lib.import_ciphertext(x, SCALE) for x in xs]
    blk = lib.new_linear_transform_blocks(ids)
    outs = lib.evaluate_linear_transform_blocks(blk, cts, rescale=rescale)
    got = [lib.export_ciphertext(o) for o in outs]
    _delete(lib, cts + outs)
    assert len(got) == 2 and all(g.shape[0] == B for g in got)
    for b in range(B):
        c1 = [lib.import_ciphertext(x[b:b + 1], SCALE) for x in xs]
        o1 = lib.evaluate_linear_transform_blocks(blk, c1, rescale=rescale)
        for i in range(2):
            assert np.array_equal(got[i][b], lib.export_ciphertext(o1[i])[0]), (b, i)
        _delete(lib, c1 + o1)
    lib.delete_linear_transform_blocks(blk)


# ---- 5. whole pass -----------------------------------------------------------------------
def test_lola_n13_batch_6_matches_cpu_oracle_replay(torch_cuda):
    """The recorded LoLA stream at N = 2^13 on six encryptions of its input
    (six different ciphertexts) as one batch: every image bit for bit the CPU
    oracle's replay of that image (about half a second of CPU each)."""
    from orion_amd.replay import OrionStream
    from oracle.replay_cpu import CpuStream
    st = OrionStream("lola_n13", seed=13)
    lib = st.lib
    try:
        st.keygen()
        st.compile()
        gels = {g for h in st.lt_map.values() for g in lib.GetLinearTransformRotationKeys(h)}
        gels |= {int(lib.GaloisElement(e["args"][1])) for e in st.trace["events"]
                 if e["phase"] == "forward" and e["op"] in ("RotateNew", "Rotate")}
        cpu = CpuStream("lola_n13")
        cpu.sk = lib.export_secret_key()
        cpu.rlk = lib.export_relin_key()
        cpu.compile_keys = False
        cpu.gks = {g: lib.export_galois_key(g) for g in sorted(gels) if g != 1}  # (1: the zero rotation)
        cpu.compile()
        B = 6
        ct = st.encrypt_batch(np.stack([st.reference_input()] * B))
        x = lib.export_ciphertext(ct)
        assert x.shape[0] == B and not np.array_equal(x[0], x[B - 1])
        out = lib.export_ciphertext(st.forward(ct))
        enc = [e for e in cpu.trace["events"] if e["phase"] == "input" and e["op"] == "Encode"][0]
        for b in range(B):
            ref = cpu.forward((x[b], x.shape[2] - 1, float(enc["args"][2])))
            assert np.array_equal(out[b], ref[0]), b
    finally:
        lib.DeleteScheme()


# ---- 6. the 61-bit fallback ----------------------------------------------------------------
@pytest.fixture
def env61(torch_cuda, oracle_mod):
    """One 61-bit special prime: its limb takes the products of whole words
    reduced every 8 babies, the path for moduli above 60 bits."""
    chain = PLANT_CHAINS["k1"]

    def make():
        lib, made = _scheme(chain, 178, lambda lib, rng: {"sparse": _gen(lib, rng, SPARSE, 3)})
        orc = oracle_mod.Oracle(chain["logn"], lib.moduli(), len(chain["logq"]), len(chain["logp"]))
        return lib, orc, made

    return _cache61.get(make)


def test_61_bit_special_prime(env61):
    lib, orc, lts = env61
    t = lts["sparse"]
    assert int(lib.moduli()[lib.L]).bit_length() == 61
    B = 5
    x = _planted(lib, 3, B, 450)
    got, alone = _batch_and_alone(lib, t, x)
    for b in range(B):
        assert np.array_equal(got[b], alone[b]), b
    assert np.array_equal(got[B - 1], _oracle_lt(lib, orc, t, SPARSE, 3, x[B - 1]))
