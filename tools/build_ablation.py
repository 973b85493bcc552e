"""Build timing-only variants of liborion_hip.so (never shipped).

Usage: python tools/build_ablation.py name=FLAGS [name=FLAGS ...]
  e.g.   python tools/build_ablation.py o2="-O2"
Each variant is built with the product's flags plus FLAGS into
orion_amd/_build/liborion_hip_<name>.so (tools/ab.sh TAG lib product <name>).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orion_amd import build  # noqa: E402

if len(sys.argv) < 2 or any("=" not in a for a in sys.argv[1:]):
    sys.exit(__doc__)
for name, flags in (a.split("=", 1) for a in sys.argv[1:]):
    out = build.build(extra_flags=flags.split(), lib=os.path.join(build.BUILD, f"liborion_hip_{name}.so"),
                      build_dir=os.path.join(build.BUILD, name))
    print(out)
