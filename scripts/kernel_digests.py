#!/usr/bin/env python3
"""Digest of the gfx950 code of every kernel and device function in pt_kernels.hip and pt_kernels_fma.hip.

Compiles each translation unit device-only to assembly with the Makefile's code-generation flags and hashes each function's
body (comments dropped, basic-block label numbers normalised, so adding a function elsewhere does not move the digest of another).  Used by
tests/test_denoise_cpu.py to show that a change leaves the code of existing kernels byte for byte as it was:

    python scripts/kernel_digests.py > digests.json
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = ("pt_kernels.hip", "pt_kernels_fma.hip")


def listing(unit, out_dir):
    out = os.path.join(out_dir, unit + ".s")
    inc = ["-I" + os.path.join(ROOT, d) for d in ("include", "cuda-pathtracer_amd/host", "cuda-pathtracer_amd/csrc")]
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
                           "-fno-vectorize", *inc, "-x", "hip", "--cuda-device-only", "-S", "-o", out,
                           os.path.join(ROOT, "cuda-pathtracer_amd", "csrc", unit)])
    with open(out) as f:
        return f.read()


def function_digests(text):
    """{symbol: sha256 of its normalised body} for every function of a listing."""
    out = {}
    for m in re.finditer(r"^([A-Za-z_][\w.$]*):\s*(?:;.*)?$\n", text, re.M):
        name = m.group(1)
        if name.startswith(".L"):
            continue
        end = text.find(".Lfunc_end", m.end())
        if end < 0:
            continue
        nxt = re.search(r"^[A-Za-z_][\w.$]*:\s*(?:;.*)?$", text[m.end():end], re.M)
        if nxt:   # a data symbol, not a function
            continue
        body = re.sub(r"\s*;.*$", "", text[m.end():end], flags=re.M)   # comments name blocks by number too
        body = re.sub(r"\.L(BB|tmp)\d+_", r".L\1_", body)
        body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", body)
        out[name] = hashlib.sha256(body.encode()).hexdigest()[:32]
    return out


def digests():
    with tempfile.TemporaryDirectory() as d:
        return {unit: function_digests(listing(unit, d)) for unit in UNITS}


if __name__ == "__main__":
    json.dump(digests(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
