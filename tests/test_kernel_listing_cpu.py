"""scripts/kernel_listing.py, on the CPU: a unit is compiled once per process, and the listing reads as the tests expect.
The unit is csrc/pt_refit.hip, the smallest one."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402


def test_a_unit_is_compiled_once_and_its_metadata_names_the_refit_kernels(monkeypatch):
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    calls = []
    run = kernel_listing.subprocess.run
    monkeypatch.setattr(kernel_listing, "_listings", {})   # (whatever the process has compiled so far comes back afterwards)
    monkeypatch.setattr(kernel_listing.subprocess, "run", lambda cmd, *a, **kw: (calls.append(cmd), run(cmd, *a, **kw))[1])
    first = kernel_listing.listing("pt_refit.hip")
    assert kernel_listing.listing("pt_refit.hip") is first
    compiles = [c for c in calls if c[0] != "make"]   # (the flags are asked of `make -s hipflags`)
    assert len(compiles) == 1 and "-S" in compiles[0] and "-ffp-contract=off" in compiles[0], calls
    meta = kernel_listing.all_metadata(first)
    assert len(meta) == 4 and all(re.fullmatch(r"_ZN5ptamd\d+pt_refit_\w+", n) for n in meta), sorted(meta)
    for n, m in meta.items():
        assert m == kernel_listing.metadata(first, n) and "private_segment_fixed_size" in m and "vgpr_count" in m, (n, m)
        assert kernel_listing.body(first, n).startswith("\n" + n + ":")
