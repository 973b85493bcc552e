"""GPU tests of OrionHipStackCiphertexts / OrionHipSliceCiphertext: batch
handles made from ciphertexts that already live on the device, and taken apart
again.  Every comparison is bit for bit against the canonical host exports
(numpy concatenation / row selection), so no tolerance is involved.

* layout, a repeated handle, level and scale carried over, sources untouched;
* a source whose planes are allocated for more limbs than its level (after
  ModDropCiphertext): it is addressed by its strides;
* every (first, count) slice of a batch, and slice(stack(xs), i) == xs[i];
* more output images than one launch's source table holds, and a slice that
  straddles the launch boundary;
* refusals (bad arguments, level / scale mismatch, inside a graph capture):
  an error naming the cause and no new handle;
* through the real kernels: separately encrypted images stacked, one batched
  forward pass, outputs sliced apart == each image's own single-image pass
  (LoLA N=2^13, Standard and ConjugateInvariant ring);
* across pipeline contexts: the scheme's thread stacks two handles owned by
  two worker threads' contexts, which delete them right afterwards.
"""
import numpy as np
import pytest

from tests.helpers import SMALL, rand_ct, SchemeCache

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** 40


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_small_cache = SchemeCache()


@pytest.fixture
def small(torch_cuda):
    """function-scoped view of a module-wide scheme, rebuilt if another test
    replaced the process-global scheme (order-independent)"""

    def make():
        from orion_amd.backend import HipLibrary
        lib = HipLibrary().new_scheme(SMALL["logn"], SMALL["logq"], SMALL["logp"], 40, h=192, seed=4321)
        return lib, lib.moduli()

    return _small_cache.get(make)


def _delete(lib, handles):
    for h in handles:
        lib.DeleteCiphertext(h)


def test_stack_layout(small):
    lib, mods = small
    rng = np.random.default_rng(101)
    level = 4
    xs = [rand_ct(rng, mods, level, lib.N, B=B) for B in (1, 2, 1, 3)]
    a, b, c, d = hs = [lib.import_ciphertext(x, SCALE) for x in xs]
    s = lib.stack_ciphertexts([a, b, c, d, b])  # one handle twice
    assert lib.GetCiphertextBatch(s) == 9
    assert lib.GetCiphertextLevel(s) == level
    assert lib.GetCiphertextScaleF(s) == SCALE
    assert np.array_equal(lib.export_ciphertext(s), np.concatenate(xs + [xs[1]]))
    for h, x in zip(hs, xs):  # the sources are only read
        assert np.array_equal(lib.export_ciphertext(h), x)
        assert lib.GetCiphertextLevel(h) == level and lib.GetCiphertextScaleF(h) == SCALE
    _delete(lib, hs + [s])


def test_stack_source_allocated_for_a_higher_level(small):
    """a ciphertext dropped from level 4 to 3 keeps planes allocated for 5
    limbs (limb stride unchanged, component stride 5 limbs) and its scale"""
    lib, mods = small
    rng = np.random.default_rng(102)
    x4 = rand_ct(rng, mods, 4, lib.N, B=2)
    x3 = rand_ct(rng, mods, 3, lib.N, B=1)
    a = lib.import_ciphertext(x4, SCALE)
    lib.ModDropCiphertext(a)
    assert lib.GetCiphertextLevel(a) == 3 and lib.GetCiphertextScaleF(a) == SCALE
    b = lib.import_ciphertext(x3, SCALE)
    ea, eb = lib.export_ciphertext(a), lib.export_ciphertext(b)
    assert np.array_equal(ea, x4[:, :, :4]) and np.array_equal(eb, x3)
    s = lib.stack_ciphertexts([a, b, a])
    assert lib.GetCiphertextLevel(s) == 3 and lib.GetCiphertextBatch(s) == 5
    assert np.array_equal(lib.export_ciphertext(s), np.concatenate([ea, eb, ea]))
    t = lib.slice_ciphertext(a, 1, 1)  # the slice reads the same strides
    assert np.array_equal(lib.export_ciphertext(t), ea[1:2])
    _delete(lib, [a, b, s, t])


def test_slice(small):
    lib, mods = small
    rng = np.random.default_rng(103)
    level = 2
    x = rand_ct(rng, mods, level, lib.N, B=4)
    h = lib.import_ciphertext(x, SCALE)
    for first in range(4):
        for count in range(1, 4 - first + 1):
            t = lib.slice_ciphertext(h, first, count)
            assert lib.GetCiphertextBatch(t) == count
            assert lib.GetCiphertextLevel(t) == level and lib.GetCiphertextScaleF(t) == SCALE
            assert np.array_equal(lib.export_ciphertext(t), x[first:first + count]), (first, count)
            lib.DeleteCiphertext(t)
    assert np.array_equal(lib.export_ciphertext(h), x)
    one = lib.import_ciphertext(x[2:3], SCALE)
    t = lib.slice_ciphertext(one, 0)  # count defaults to 1
    assert np.array_equal(lib.export_ciphertext(t), x[2:3])
    singles = [lib.import_ciphertext(x[i:i + 1], SCALE) for i in range(4)]
    s = lib.stack_ciphertexts(singles)
    for i in range(4):
        u = lib.slice_ciphertext(s, i, 1)
        assert np.array_equal(lib.export_ciphertext(u), x[i:i + 1]), i
        lib.DeleteCiphertext(u)
    _delete(lib, [h, one, t, s] + singles)


def test_more_images_than_one_launch(small):
    """T + 3 single images: two launches; a slice across the launch boundary"""
    from orion_amd.backend import STACK_TABLE_SIZE as T
    lib, mods = small
    rng = np.random.default_rng(104)
    n = T + 3
    x = rand_ct(rng, mods, 1, lib.N, B=n)
    hs = [lib.import_ciphertext(x[i:i + 1], SCALE) for i in range(n)]
    s = lib.stack_ciphertexts(hs)
    assert lib.GetCiphertextBatch(s) == n
    assert np.array_equal(lib.export_ciphertext(s), x)
    t = lib.slice_ciphertext(s, T - 1, 3)
    assert np.array_equal(lib.export_ciphertext(t), x[T - 1:T + 2])
    w = lib.slice_ciphertext(s, 1, T + 1)  # a slice of more images than one launch holds
    assert np.array_equal(lib.export_ciphertext(w), x[1:T + 2])
    _delete(lib, hs + [s, t, w])


def test_refusals(small):
    lib, mods = small
    rng = np.random.default_rng(105)
    x = rand_ct(rng, mods, 3, lib.N, B=2)
    a = lib.import_ciphertext(x, SCALE)
    b = lib.import_ciphertext(x, SCALE)
    lo = lib.import_ciphertext(x[:, :, :3], SCALE)  # level 2
    other = lib.import_ciphertext(x, SCALE)
    lib.SetCiphertextScale(other, 2 ** 41)
    live = sorted(lib.GetLiveCiphertexts())
    unknown = max(live) + 1000

    def refused(match, fn, *args):
        with pytest.raises(RuntimeError, match=match):
            fn(*args)
        assert sorted(lib.GetLiveCiphertexts()) == live, match

    refused("at least one", lib.stack_ciphertexts, [])
    refused(f"handle not found: {unknown}", lib.stack_ciphertexts, [a, unknown])
    refused(f"handle not found: {unknown}", lib.slice_ciphertext, unknown, 0, 1)
    refused(rf"{a} \(level 3\) and {lo} \(level 2\): the levels differ", lib.stack_ciphertexts, [a, b, lo])
    refused(rf"{a} \(scale 1099511627776\) and {other} \(scale 2199023255552\): the scales differ",
            lib.stack_ciphertexts, [a, other])
    refused("slice of 0 images", lib.slice_ciphertext, a, 0, 0)
    refused("starts at image -1", lib.slice_ciphertext, a, -1, 1)
    refused(rf"images 1\.\.2 of ciphertext {a}, whose batch is 2", lib.slice_ciphertext, a, 1, 2)
    refused(rf"images 0\.\.2 of ciphertext {a}, whose batch is 2", lib.slice_ciphertext, a, 0, 3)
    lib.OrionHipGraphBegin()
    clone = None
    try:
        refused("OrionHipStackCiphertexts is not allowed while capturing", lib.stack_ciphertexts, [a, b])
        refused("OrionHipSliceCiphertext is not allowed while capturing", lib.slice_ciphertext, a, 0, 1)
        clone = lib.CloneCiphertext(a)  # (the capture records something)
    finally:
        gid = lib.OrionHipGraphEnd()
    lib.OrionHipGraphDestroy(gid)
    # the library is usable afterwards
    s = lib.stack_ciphertexts([a, b])
    assert np.array_equal(lib.export_ciphertext(s), np.concatenate([x, x]))
    _delete(lib, [a, b, lo, other, s] + ([clone] if clone is not None else []))


def _single_pass(st, h):
    """forward() of a clone of h alone: its exported output"""
    lib = st.lib
    c = lib.CloneCiphertext(h)
    o = st.forward(c)
    ref = lib.export_ciphertext(o)
    lib.DeleteCiphertext(o)
    if o != c:
        lib.DeleteCiphertext(c)
    return ref


@pytest.mark.parametrize("name", ["lola_n13", "lola_n13_ci"])
def test_forward_stacked_matches_single_image_passes(torch_cuda, name):
    from orion_amd.replay import OrionStream
    st = OrionStream(name, seed=61)
    lib = st.lib
    try:
        st.keygen()
        st.compile()
        rng = np.random.default_rng(62)
        imgs = rng.standard_normal((3,) + np.asarray(st.reference_input()).shape[1:]).astype(np.float32)
        cts = st.encrypt_images(imgs)
        assert len(cts) == 3 and all(lib.GetCiphertextBatch(c) == 1 for c in cts)
        xs = [lib.export_ciphertext(c) for c in cts]
        refs = [_single_pass(st, c) for c in cts]
        outs = st.forward_stacked(cts)
        assert len(outs) == 3
        for i, (o, ref) in enumerate(zip(outs, refs)):
            assert lib.GetCiphertextBatch(o) == 1
            assert np.array_equal(lib.export_ciphertext(o), ref), i
        for c, x in zip(cts, xs):  # the inputs are alive and unchanged
            assert np.array_equal(lib.export_ciphertext(c), x)
        assert sorted(lib.GetLiveCiphertexts()) == sorted(cts + outs)
    finally:
        lib.DeleteScheme()


def test_stack_across_pipeline_contexts(torch_cuda):
    from orion_amd.replay import OrionStream, Pipelines
    st = OrionStream("lola_n13", seed=63)
    lib = st.lib
    try:
        st.keygen()
        st.compile()
        rng = np.random.default_rng(64)
        imgs = rng.standard_normal((2,) + np.asarray(st.reference_input()).shape[1:]).astype(np.float32)
        own = st.encrypt_images(imgs)
        xs = [lib.export_ciphertext(c) for c in own]
        scale = lib.GetCiphertextScaleF(own[0])
        refs = [_single_pass(st, c) for c in own]  # before the pipelines exist
        pipes = Pipelines(lib, 2, device=0)
        try:
            theirs = pipes.run([(lambda x=x: lib.import_ciphertext(x, scale)) for x in xs])
            assert [c >> 20 for c in theirs] == pipes.contexts
            s = lib.stack_ciphertexts(theirs)  # the scheme's thread reads two foreign handles
            pipes.run([(lambda c=c: lib.DeleteCiphertext(c)) for c in theirs])  # at once: the owners delete them
            assert s >> 20 == 0
            assert lib.GetCiphertextBatch(s) == 2
            assert np.array_equal(lib.export_ciphertext(s), np.concatenate(xs))
            out = lib.export_ciphertext(st.forward(s))
            for i in range(2):
                assert np.array_equal(out[i:i + 1], refs[i]), i
        finally:
            pipes.close()
    finally:
        lib.DeleteScheme()
