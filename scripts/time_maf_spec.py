"""Time the host-side image builders of ``pocomc_amd/maf_spec.py`` (CPU only, no GPU and no library needed): what
``Flow()`` pays per construction for its gather maps.

    python scripts/time_maf_spec.py [--parent PATH/TO/OTHER/maf_spec.py] [--out profiles/maf_spec_build.txt]

Per spec of ``tests/test_maf_spec_images_cpu.py`` and per builder (``pack_index``, ``pack_index_bf16``, ``wide_index``,
``train_index`` without its cache): milliseconds per call, median of ``--calls`` calls [min .. max], single thread.  With
``--parent`` the same is measured for another ``maf_spec.py`` (a checkout of the parent commit's), its calls interleaved with
the tree's so that both see the same machine, and every line ends in the verdict of the rule

    median(tree) <= median(parent) + (max(parent) - min(parent))

the parent's own spread being the margin of a sub-second timing on a shared CPU.  Exit status 1 if a line misses it."""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_maf_spec_images_cpu import SPECS                  # noqa: E402

BUILDERS = ("pack_index", "pack_index_bf16", "wide_index", "train_index")


def load(path, name):
    mod_spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(mod_spec)
    sys.modules[name] = mod                                 # (dataclasses looks the module up while the class is built)
    mod_spec.loader.exec_module(mod)
    return mod.MAFSpec


def call_ms(spec, builder):
    spec._train_index = None                                # train_index: the build, not the cache
    t0 = time.perf_counter()
    getattr(spec, builder)()
    return (time.perf_counter() - t0) * 1e3


def fmt(t):
    return f"{np.median(t):9.2f} [{min(t):.2f} .. {max(t):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="another maf_spec.py to time alongside the tree's")
    ap.add_argument("--parent-commit", default="?", help="the commit --parent was taken from, for the header")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--spec", action="append", default=None, help="only this spec (may be repeated); default: all")
    a = ap.parse_args()
    classes = [("tree", load(os.path.join(ROOT, "pocomc_amd", "maf_spec.py"), "maf_spec_tree"))]
    if a.parent:
        classes.insert(0, ("parent", load(a.parent, "maf_spec_parent")))
    lines = [f"# MAFSpec image builders, ms per call on one CPU thread: median of {a.calls} calls [min .. max]"
             + (f"; parent = maf_spec.py of {a.parent_commit}; last column: median(parent) / median(tree), and ok where "
                "median(tree) <= median(parent) + (max(parent) - min(parent))" if a.parent else ""),
             "# spec            builder          | " + " | ".join(f"{who:>28s}" for who, _ in classes)]
    print("\n".join(lines), flush=True)
    missed = 0
    for key, (args, kw) in SPECS.items():
        if a.spec and key not in a.spec:
            continue
        specs = [cls(*args, **kw) for _, cls in classes]
        for builder in BUILDERS:
            for s in specs:
                call_ms(s, builder)                         # warm-up: imports, the allocator
            t = [[] for _ in specs]
            for _ in range(a.calls):
                for k, s in enumerate(specs):
                    t[k].append(call_ms(s, builder))
            line = f"{key:15s}   {builder:16s} | " + " | ".join(f"{fmt(x):>28s}" for x in t)
            if a.parent:
                ok = np.median(t[1]) <= np.median(t[0]) + (max(t[0]) - min(t[0]))
                missed += not ok
                line += f" | {np.median(t[0]) / np.median(t[1]):6.1f}x {'ok' if ok else 'SLOWER'}"
            lines.append(line)
            print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(1 if missed else 0)


if __name__ == "__main__":
    main()
