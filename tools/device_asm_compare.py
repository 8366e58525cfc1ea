#!/usr/bin/env python
"""Shows that a host-side change left the device code alone: the gfx950 assembly of every kernel source, compiled with
the file's own flags_for() flags, from two trees.

    python tools/device_asm_compare.py dump <csrc dir of a tree> <out dir>
        writes <out dir>/shipped/<source>.s and <out dir>/variants/<source>.s (-DSGR_WITH_VARIANTS=1, which adds
        csrc/variants/*.hip and the `#if SGR_WITH_VARIANTS` parts) -- without the lines naming __hip_cuid_<hash>, the
        one symbol that differs between two compiles of the same file
    python tools/device_asm_compare.py compare <out dir A> <out dir B> <report.txt>
        one line per (build, source): identical / DIFFERENT; exit status 1 on any difference
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from street_gaussians_amd import build as b  # noqa: E402

BUILDS = {"shipped": (b.SOURCES, []), "variants": (b.SOURCES + b.VARIANT_SOURCES, ["-DSGR_WITH_VARIANTS=1"])}


def dump(csrc, out):
    def one(job):
        build, src, extra = job
        dst = os.path.join(out, build, src.replace(os.sep, "_").replace(".hip", ".s"))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        text = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + b.flags_for(src) + extra +
                              ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", "-"],
                              check=True, capture_output=True, text=True).stdout
        with open(dst, "w") as f:
            f.writelines(line for line in text.splitlines(True) if "__hip_cuid_" not in line)

    jobs = [(build, src, extra) for build, (sources, extra) in BUILDS.items() for src in sources]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(one, jobs))


def compare(a, c, report):
    lines, bad = [], 0
    for build, (sources, _) in BUILDS.items():
        for src in sources:
            name = os.path.join(build, src.replace(os.sep, "_").replace(".hip", ".s"))
            ta, tc = open(os.path.join(a, name)).read(), open(os.path.join(c, name)).read()
            bad += ta != tc
            lines.append(f"{build:9s} {src:34s} {len(tc.splitlines()):7d} lines  {'identical' if ta == tc else 'DIFFERENT'}")
    lines.append(f"{bad} of {len(lines)} device assembly texts differ")
    with open(report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4]))
