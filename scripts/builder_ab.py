#!/usr/bin/env python3
"""Host build time of the atrium's tree with every node form, two builds of libptamd.so alternating (CPU only).

  python scripts/builder_ab.py <libptamd.so A> <libptamd.so B> [--runs 5]

Every run is a fresh process that loads one library and times one ptamd_host_bvh8_trace call with zero rays: build_bvh with
leaves of at most two faces and all forms, nothing else.  Prints one line per run and the mean and spread of both series."""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(lib_path, faces_path):
    lib = ctypes.CDLL(lib_path)
    faces = np.fromfile(faces_path, dtype=np.uint8)
    n = faces.size // 112   # sizeof(ptamd_face)
    t0 = time.perf_counter()
    rc = lib.ptamd_host_bvh8_trace(faces.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(n), None, ctypes.c_uint32(0), None, None)
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    print("%.4f" % dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd.synthetic import write_atrium
    with tempfile.TemporaryDirectory() as tmp:
        hs = P.HostScene.load(write_atrium(tmp))
        faces_path = os.path.join(tmp, "faces.bin")
        hs.faces.tofile(faces_path)
        print("atrium: %d faces, leaves of at most 2, all forms; seconds per build" % len(hs.faces))
        series = {lib: [] for lib in args.libs}
        for run in range(args.runs):
            for label, lib in zip("AB", args.libs):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, faces_path], capture_output=True, text=True, check=True)
                series[lib].append(float(out.stdout))
                print("run %d  %s  %.4f" % (run, label, series[lib][-1]), flush=True)
    for label, lib in zip("AB", args.libs):
        v = series[lib]
        print("%s  %s  mean %.4f  min %.4f  max %.4f" % (label, lib, sum(v) / len(v), min(v), max(v)))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
