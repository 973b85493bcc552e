"""Stack / slice microbenchmark at LoLA's input shape (N=2^15, level 5, 64
single-image ciphertexts; chain of tests/golden/lola_n15_trace.json).  In one
run, alternating per repetition, it times with HIP events on the library
stream:

  new   one stack_ciphertexts call over the 64 handles, and 64
        slice_ciphertext calls on the result (OrionHipStackCiphertexts /
        OrionHipSliceCiphertext: one gather kernel launch per call);
  old   the route without them, for the same two jobs: export_ciphertext_device
        per handle -> torch.cat -> import_ciphertext_device (2 (level+1) strided
        2-D copies per call and image), and export_ciphertext_device of the
        batch -> import_ciphertext_device per image.

Both routes' results are compared with the source data bit for bit first.
The gather kernel alone is timed by the library's own profiler (category
elementwise, HIP events around the launch) and priced at its algorithmic
bytes, 16 N per limb-image, against the 6.3 TB/s achievable HBM rate.
Prints one JSON object (and writes it to --out).
Usage: python tools/stack_ubench.py [--images 64] [--warmup 5] [--reps 30] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orion_amd.backend import STACK_TABLE_SIZE, HipLibrary  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s


def measure(torch, lib, a, cfg, level):
    """(per-repetition ms of the four routes, the profiler's elementwise
    record).  Every tensor, event and stream object made here is released on
    return, while the library stream they were recorded on still exists."""
    B, nl, N = a.images, level + 1, lib.N
    scale = 2.0 ** cfg["logscale"]
    # residues below 2^39 are reduced under every modulus of the chain; a copy's speed does not depend on them
    gen = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randint(0, 1 << 39, (B, 2, nl, N), dtype=torch.int64, device="cuda", generator=gen)
    torch.cuda.synchronize()
    hs = [lib.import_ciphertext_device(data[i:i + 1], scale) for i in range(B)]
    lib_s = lib._streams(data)[1]

    def new_stack():
        return lib.stack_ciphertexts(hs)

    def new_slices(s):
        return [lib.slice_ciphertext(s, i, 1) for i in range(B)]

    def old_stack():
        parts = [lib.export_ciphertext_device(h, torch.empty((1, 2, nl, N), dtype=torch.int64, device="cuda"))
                 for h in hs]
        return lib.import_ciphertext_device(torch.cat(parts), scale)

    def old_slices(s):
        whole = lib.export_ciphertext_device(s, torch.empty((B, 2, nl, N), dtype=torch.int64, device="cuda"))
        return [lib.import_ciphertext_device(whole[i:i + 1], scale) for i in range(B)]

    def exported(h):
        n = lib.GetCiphertextBatch(h)
        return lib.export_ciphertext_device(h, torch.empty((n, 2, nl, N), dtype=torch.int64, device="cuda"))

    def drop(x):
        for h in (x if isinstance(x, list) else [x]):
            lib.DeleteCiphertext(h)

    # every call below runs with the library stream as torch's current stream,
    # so one pair of events on that stream brackets a whole route
    with torch.cuda.stream(lib_s):
        for stack, slices in ((new_stack, new_slices), (old_stack, old_slices)):  # results first
            s = stack()
            assert torch.equal(exported(s), data), stack.__name__
            parts = slices(s)
            for i, p in enumerate(parts):
                assert torch.equal(exported(p), data[i:i + 1]), (slices.__name__, i)
            drop(parts)
            drop(s)

        def timed(fn, *args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(lib_s)
            r = fn(*args)
            e1.record(lib_s)
            e1.synchronize()
            return e0.elapsed_time(e1), r

        ms = {k: [] for k in ("new_stack", "new_slices", "old_stack", "old_slices")}
        for rep in range(a.warmup + a.reps):
            t_ns, s = timed(new_stack)
            t_nl, parts = timed(new_slices, s)
            drop(parts)
            drop(s)
            t_os, s = timed(old_stack)
            t_ol, parts = timed(old_slices, s)
            drop(parts)
            drop(s)
            if rep >= a.warmup:
                for k, v in zip(ms, (t_ns, t_nl, t_os, t_ol)):
                    ms[k].append(v)
        # the kernel alone: the library's profiler brackets each launch with events
        lib.OrionHipSynchronize()
        lib.OrionHipProfileReset()
        lib.OrionHipProfile(1 << 2)
        for _ in range(a.reps):
            drop(new_stack())
        lib.OrionHipProfile(0)
        ker = lib.profile_read()["elementwise"]
        drop(hs)
    lib.OrionHipSynchronize()
    torch.cuda.synchronize()
    return ms, ker


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("stack_ubench needs a GPU (no CPU fallback)")
    with open(os.path.join(ROOT, "tests", "golden", "lola_n15_trace.json")) as f:
        meta = json.load(f)["meta"]
    cfg, level = meta["config"], meta["input_level"]
    lib = HipLibrary().new_scheme(cfg["logn"], cfg["logq"], cfg["logp"], cfg["logscale"], h=cfg["h"], seed=5, device=0)
    B, nl, N = a.images, level + 1, lib.N
    # The scheme is left to the library's teardown at exit, as bench.py leaves
    # it: DeleteScheme destroys the library stream, and torch's caching
    # allocator still names that stream in the blocks of the tensors used here
    # (record_stream, allocations made with it current).
    ms, ker = measure(torch, lib, a, cfg, level)

    def stat(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med = {k: statistics.median(v) for k, v in ms.items()}
    kbytes = 16.0 * N * 2 * nl * B
    per_call = -(-B // STACK_TABLE_SIZE)  # launches per stack call
    assert ker["launches"] == a.reps * per_call and ker["bytes"] == kbytes * a.reps, ker
    kms = ker["ms"] / a.reps
    out = {
        "bench": "stack_ubench", "logn": cfg["logn"], "level": level, "images": B, "warmup": a.warmup, "reps": a.reps,
        "timer": "HIP events on the library stream around each route, median of reps",
        "new": {"stack_1_call": stat(ms["new_stack"]), "slice_%d_calls" % B: stat(ms["new_slices"])},
        "old": {"export_x%d_cat_import" % B: stat(ms["old_stack"]), "export_import_x%d" % B: stat(ms["old_slices"]),
                "copies_per_direction": 2 * nl * B},
        "ratio_old_over_new": {"stack": round(med["old_stack"] / med["new_stack"], 2),
                               "slices": round(med["old_slices"] / med["new_slices"], 2),
                               "both": round((med["old_stack"] + med["old_slices"]) /
                                             (med["new_stack"] + med["new_slices"]), 2)},
        "kernel": {"name": "gather_images_kernel", "launches": ker["launches"], "ms_per_stack_call": round(kms, 5),
                   "algorithmic_bytes_per_stack_call": kbytes, "bytes_per_s": round(kbytes / (kms * 1e-3), 1),
                   "share_of_achievable_hbm_6.3TBps": round(kbytes / (kms * 1e-3) / HBM_ACHIEVABLE, 4)},
    }
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
