"""Compare the gfx950 code of every kernel between two source trees (no GPU).

Usage: python tools/isa_diff.py OLD_TREE NEW_TREE [--jobs N] [--keep DIR]

Each .hip file of orion_amd/csrc is compiled device-only to assembly with the
flags of orion_amd/build.py.  Per kernel symbol the tool prints "identical" or
"differs" (the text between the symbol's label and its end label, comments
dropped and local label numbers normalised) and, beside it, VGPRs, AGPRs,
SGPRs, scratch and LDS bytes from the code object's metadata.  It compares
text only.  Exit status 1 when a kernel present in both trees differs in code
or resources; kernels present in one tree only are listed.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off",
         "--offload-device-only", "-S", "-w"]
RES = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"),
       ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size")]


def compile_tree(tree, out, jobs):
    csrc = os.path.join(tree, "orion_amd", "csrc")
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    os.makedirs(out, exist_ok=True)

    def run(src):
        asm = os.path.join(out, src + ".s")
        r = subprocess.run([HIPCC] + FLAGS + [os.path.join(csrc, src), "-o", asm],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"compile failed: {tree}/{src}\n{r.stderr}")
        return src, asm

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        return dict(ex.map(run, srcs))


def parse(asm):
    """{kernel symbol: (normalised body text, {resource: value})}"""
    with open(asm) as f:
        lines = f.read().split("\n")
    text = "\n".join(lines)
    meta = {}
    m = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", text, re.S | re.M)
    for chunk in re.split(r"^  - ", m.group(1) if m else "", flags=re.M)[1:]:
        chunk = "    " + chunk  # the list marker stood where the first key's indent is
        name = re.search(r"^    \.name:\s+(\S+)", chunk, re.M).group(1)
        meta[name] = {k: int(re.search(rf"^    \{key}:\s+(\d+)", chunk, re.M).group(1))
                      for k, key in RES}
    label = {ln.split(":", 1)[0]: i for i, ln in enumerate(lines) if ln[:1] not in ("", "\t", " ", ".", ";")}
    out = {}
    for name, res in meta.items():
        start = label[name]
        body = []
        for ln in lines[start + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = ln.split(";", 1)[0].rstrip()
            if ln:
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        out[name] = ("\n".join(body), res)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.split("\n")))


def fmt(res):
    return " ".join(f"{k}={res[k]}" for k, _ in RES)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", help="keep the assembly files in this directory")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    try:
        old = compile_tree(a.old, os.path.join(tmp, "old"), a.jobs)
        new = compile_tree(a.new, os.path.join(tmp, "new"), a.jobs)
        bad = n_same = 0
        for src in sorted(set(old) | set(new)):
            ko = parse(old[src]) if src in old else {}
            kn = parse(new[src]) if src in new else {}
            pretty = demangle(sorted(set(ko) | set(kn)))
            print(f"== {src}: {len(ko)} kernels before, {len(kn)} after")
            for sym in sorted(pretty, key=pretty.get):
                if sym not in kn:
                    print(f"gone       {pretty[sym]}  [{fmt(ko[sym][1])}]")
                elif sym not in ko:
                    print(f"new        {pretty[sym]}  [{fmt(kn[sym][1])}]")
                elif ko[sym] == kn[sym]:
                    n_same += 1
                    print(f"identical  {pretty[sym]}  [{fmt(kn[sym][1])}]")
                else:
                    bad += 1
                    word = "differs  " if ko[sym][0] != kn[sym][0] else "resources"
                    print(f"{word}  {pretty[sym]}  [{fmt(ko[sym][1])}] -> [{fmt(kn[sym][1])}]")
        print(f"== {n_same} identical, {bad} differ")
        return 1 if bad else 0
    finally:
        if not a.keep:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
