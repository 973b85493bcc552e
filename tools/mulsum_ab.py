"""A/B of OrionHipMulRelinSum against the loop of existing calls it replaces.

On LoLA's chain (N = 2^15, logQ = [60] + [40] x 11, logP = [60, 60]), at levels
5 and 11, batch 1 and 64, n = 2, 4, 8, 16 pairs of distinct ciphertexts:
  fused: one OrionHipMulRelinSum(a, b, n);
  loop:  MulRelinCiphertextNew(a[i], b[i]) for each pair, AddCiphertext into
         the first product, the other products deleted (the unchanged path).
Either leaves its last ModDown pending (the library's deferral), so each timed
region ends with one call that changes nothing and lets the pending ModDown
run: both regions hold everything up to the finished sum.

Timing: HIP events on the library's stream around each region, both variants
warmed first, then interleaved fused, loop, fused, loop, ...; the median of the
repetitions.  Below each line the launches and the profiled kernel time per
kernel family of one more repetition of each variant (OrionHipProfile, a run
of its own: profiling adds events around every launch).

With --against OTHER.so (the library of another build, tools/build_commit_lib.sh)
the n = 1 rows run instead: the plain product, MulRelinCiphertextNew(a, b), of
this tree's library (new) against OTHER's (old), and OTHER against a second
copy of itself (old2).  old2 / old is the A/A spread of a cell: what a
difference between new and old has to exceed to mean anything.  Each library
is an instance of its own with its own scheme and operands of the same seed;
all of them run on one stream, so the same method holds: warmed, interleaved
new, old, old2, new, ..., the pending ModDown inside each region, the median.

usage: python tools/mulsum_ab.py [--reps 20] [--warm 3] [--against OTHER.so] > profiles/NAME.txt
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orion_amd.backend import HipLibrary  # noqa: E402

LOGN, LOGQ, LOGP = 15, [60] + [40] * 11, [60, 60]
SCALE = float(2 ** 20)


def operands(lib, rng, level, B, count):
    """count ciphertexts of batch B with buffers of their own (one random
    image, stacked B times and cloned: the timing does not depend on the values)"""
    mods = lib.moduli()
    x = np.stack([rng.integers(0, mods[j], (1, 2, lib.N), dtype=np.uint64) for j in range(level + 1)], axis=2)
    one = lib.import_ciphertext(x, SCALE)
    first = lib.stack_ciphertexts([one] * B)
    lib.DeleteCiphertext(one)
    return [first] + [lib.CloneCiphertext(first) for _ in range(count - 1)]


def fused(lib, a, b):
    return lib.mul_relin_sum(a, b)


def loop(lib, a, b):
    acc = lib.MulRelinCiphertextNew(a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        t = lib.MulRelinCiphertextNew(x, y)
        lib.AddCiphertext(acc, t)
        lib.DeleteCiphertext(t)
    return acc


def plain_ab(args, torch):
    """the n = 1 rows (--against)"""
    tmp = tempfile.mkdtemp()
    paths = {"new": None, "old": args.against, "old2": shutil.copy(args.against, os.path.join(tmp, "liborion_hip_twin.so"))}
    stream = torch.cuda.Stream()
    libs, still = {}, {}
    for k, p in paths.items():
        lib = libs[k] = (HipLibrary(p) if p else HipLibrary()).new_scheme(LOGN, LOGQ, LOGP, 40, h=192, seed=11)
        lib.OrionHipSetStream(stream.cuda_stream)
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        lib.GenerateRelinearizationKey()
        still[k] = lib.import_ciphertext(np.zeros((1, 2, 1, lib.N), dtype=np.uint64), SCALE)

    def region(k, a, b):
        lib = libs[k]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h = lib.MulRelinCiphertextNew(a, b)
        lib.SetCiphertextScale(still[k], 1 << 20)  # changes nothing; the pending ModDown runs first
        e1.record(stream)
        lib.DeleteCiphertext(h)
        return e0, e1

    print(f"device: {torch.cuda.get_device_name(0)}   N = 2^{LOGN}  logQ = {LOGQ}  logP = {LOGP}   "
          f"MulRelinCiphertextNew, new = this tree, old = old2 = {args.against}; "
          f"median of {args.reps} interleaved repetitions after {args.warm} warm ones, HIP events")
    print("level   B    n     new ms    old ms   old2 ms   new/old   old2/old   (min .. max of each)")
    for level in args.levels:
        for B in args.batches:
            ops = {k: operands(libs[k], np.random.default_rng(12), level, B, 2) for k in libs}
            for _ in range(args.warm):
                for k in libs:
                    region(k, *ops[k])
            torch.cuda.synchronize()
            ev = {k: [] for k in libs}
            for _ in range(args.reps):
                for k in libs:
                    ev[k].append(region(k, *ops[k]))
            torch.cuda.synchronize()
            ms = {k: [e0.elapsed_time(e1) for e0, e1 in ev[k]] for k in ev}
            md = {k: statistics.median(ms[k]) for k in ms}
            print(f"{level:5d} {B:4d}    1   {md['new']:8.3f}  {md['old']:8.3f}  {md['old2']:8.3f}   "
                  f"{md['new'] / md['old']:7.3f}   {md['old2'] / md['old']:8.3f}   ("
                  + ", ".join(f"{k} {min(ms[k]):.3f} .. {max(ms[k]):.3f}" for k in ms) + ")")
            for k in ("new", "old"):
                lib = libs[k]
                lib.OrionHipSynchronize()
                lib.OrionHipProfileReset()
                lib.OrionHipProfile(1)
                h = lib.MulRelinCiphertextNew(*ops[k])
                lib.SetCiphertextScale(still[k], 1 << 20)
                lib.OrionHipSynchronize()
                lib.OrionHipProfile(0)
                lib.DeleteCiphertext(h)
                print(f"        {k:4s} " + "   ".join(f"{n} {v['launches']} launches {v['ms']:.3f} ms"
                                                      for n, v in sorted(lib.profile_read().items()) if v["launches"]))
            sys.stdout.flush()
            for k in libs:
                for h in ops[k]:
                    libs[k].DeleteCiphertext(h)
    for lib in libs.values():
        lib.DeleteScheme()
    shutil.rmtree(tmp)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="another build's liborion_hip.so: run the n = 1 rows against it")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--levels", type=int, nargs="+", default=[5, 11])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--pairs", type=int, nargs="+", default=[2, 4, 8, 16])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mulsum_ab.py needs a GPU: nothing is measured without one")
    if args.against:
        return plain_ab(args, torch)

    lib = HipLibrary().new_scheme(LOGN, LOGQ, LOGP, 40, h=192, seed=11)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    lib.GenerateRelinearizationKey()
    ptr = lib.OrionHipGetStream()
    stream = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
    rng = np.random.default_rng(12)
    still = lib.import_ciphertext(np.zeros((1, 2, 1, lib.N), dtype=np.uint64), SCALE)

    def region(fn, a, b):
        """one timed repetition: (start event, end event); the result deleted"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h = fn(lib, a, b)
        lib.SetCiphertextScale(still, 1 << 20)  # changes nothing; a pending ModDown runs first
        e1.record(stream)
        lib.DeleteCiphertext(h)
        return e0, e1

    def profiled(fn, a, b):
        lib.OrionHipSynchronize()
        lib.OrionHipProfileReset()
        lib.OrionHipProfile(1)
        h = fn(lib, a, b)
        lib.SetCiphertextScale(still, 1 << 20)
        lib.OrionHipSynchronize()
        lib.OrionHipProfile(0)
        lib.DeleteCiphertext(h)
        return {k: (v["launches"], v["ms"]) for k, v in lib.profile_read().items() if v["launches"]}

    print(f"device: {torch.cuda.get_device_name(0)}   N = 2^{LOGN}  logQ = {LOGQ}  logP = {LOGP}   "
          f"median of {args.reps} interleaved repetitions after {args.warm} warm ones, HIP events")
    print("level   B    n   fused ms   loop ms   loop/fused   (min .. max of either)")
    for level in args.levels:
        for B in args.batches:
            ops = operands(lib, rng, level, B, 2 * max(args.pairs))
            for n in args.pairs:
                a, b = ops[:n], ops[max(args.pairs):max(args.pairs) + n]
                for _ in range(args.warm):
                    for fn in (fused, loop):
                        lib.DeleteCiphertext(fn(lib, a, b))
                lib.OrionHipSynchronize()
                ev = {fused: [], loop: []}
                for _ in range(args.reps):
                    for fn in (fused, loop):
                        ev[fn].append(region(fn, a, b))
                lib.OrionHipSynchronize()
                ms = {fn: [e0.elapsed_time(e1) for e0, e1 in ev[fn]] for fn in ev}
                f, lp = statistics.median(ms[fused]), statistics.median(ms[loop])
                print(f"{level:5d} {B:4d} {n:4d}   {f:8.3f}  {lp:8.3f}   {lp / f:10.2f}   "
                      f"(fused {min(ms[fused]):.3f} .. {max(ms[fused]):.3f}, loop {min(ms[loop]):.3f} .. {max(ms[loop]):.3f})")
                pf, pl = profiled(fused, a, b), profiled(loop, a, b)
                for k in sorted(set(pf) | set(pl)):
                    nf, tf = pf.get(k, (0, 0.0))
                    nl, tl = pl.get(k, (0, 0.0))
                    print(f"        {k:14s} fused {nf:4d} launches {tf:8.3f} ms    loop {nl:4d} launches {tl:8.3f} ms")
                sys.stdout.flush()
            for h in ops:
                lib.DeleteCiphertext(h)
    lib.DeleteScheme()


if __name__ == "__main__":
    main()
