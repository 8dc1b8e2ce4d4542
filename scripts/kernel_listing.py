#!/usr/bin/env python3
"""The gfx950 assembly listing of a unit of cuda-pathtracer_amd/csrc as the Makefile compiles it, and what the tests and the
scripts beside this one read off it.  The flags are the Makefile's HIPFLAGS (`make -s hipflags`); a listing is compiled once per
process, unit and source text.

    python3 scripts/kernel_listing.py pt_refit.hip > pt_refit.s
"""
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-pathtracer_amd", "csrc")
_listings = {}


def hipcc():
    """The compiler ($HIPCC, else the Makefile's default, else the one on PATH), or None when this host has none."""
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return shutil.which("hipcc")


def listing(unit, source=None, extra=()):
    """The assembly of csrc/`unit`, compiled device-only.  source: the text to compile in the unit's place (its headers still come
    from the tree); extra: flags put in front of the Makefile's, as EXTRA_HIPFLAGS."""
    if source is None:
        with open(os.path.join(CSRC, unit)) as f:
            source = f.read()
    key = (unit, source, tuple(extra))
    if key not in _listings:
        flags = subprocess.check_output(["make", "-s", "hipflags", "EXTRA_HIPFLAGS=" + shlex.join(extra)], cwd=ROOT, text=True)
        with tempfile.TemporaryDirectory() as d:
            src, out = os.path.join(d, unit), os.path.join(d, unit + ".s")
            with open(src, "w") as f:
                f.write(source)
            done = subprocess.run([hipcc() or "hipcc", *shlex.split(flags), "-x", "hip", "--cuda-device-only", "-S", "-o", out, src],
                                  cwd=ROOT, stderr=subprocess.PIPE, text=True)   # (the flags' -I paths are relative to the root)
            if done.returncode:
                sys.stderr.write(done.stderr)
                done.check_returncode()
            with open(out) as f:
                _listings[key] = f.read()
    return _listings[key]


def metadata(text, kernel):
    """The kernel's entry in the code object's amdhsa.kernels metadata: {key: int}."""
    i = text.index(".name:           " + kernel)
    block = text[i:i + 4000].split("\n  - ")[0]
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}


def all_metadata(text):
    """{kernel: metadata} of every kernel of namespace ptamd in the listing."""
    return {n: metadata(text, n) for n in re.findall(r"\.name:\s+(_ZN5ptamd\S+)", text)}


def body(text, kernel):
    """The function's instructions, from its label to its end."""
    i = text.index("\n" + kernel + ":")
    return text[i:text.index(".Lfunc_end", i)]


if __name__ == "__main__":
    sys.stdout.write(listing(sys.argv[1]))
