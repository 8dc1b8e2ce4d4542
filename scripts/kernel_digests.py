#!/usr/bin/env python3
"""Digest of the gfx950 code of every kernel and device function in pt_kernels.hip and pt_kernels_fma.hip.

Takes each translation unit's listing as the Makefile compiles it (scripts/kernel_listing.py) and hashes each function's
body (comments dropped, basic-block label numbers normalised, so adding a function elsewhere does not move the digest of another).  Used by
tests/test_denoise_cpu.py to show that a change leaves the code of existing kernels byte for byte as it was:

    python scripts/kernel_digests.py > digests.json
"""
import hashlib
import json
import os
import re
import sys

import kernel_listing

UNITS = ("pt_kernels.hip", "pt_kernels_fma.hip")


def listing(unit, out_dir=None):
    """kernel_listing.listing(unit) in the form this script had it first: the text, and a copy in out_dir/<unit>.s"""
    text = kernel_listing.listing(unit)
    if out_dir is not None:
        with open(os.path.join(out_dir, unit + ".s"), "w") as f:
            f.write(text)
    return text


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
    return {unit: function_digests(listing(unit)) for unit in UNITS}


if __name__ == "__main__":
    json.dump(digests(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
