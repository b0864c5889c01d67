"""Build-time audit of the hand-off form (tools/audit_plain_loads.py) on the act instantiations of the resident grids,
vjf_mega_act_kernel and vjf_mega_lite_act_kernel: their waits do not acquire either, so every load of a byte another workgroup
of the launch stored must be an sc1 load.  The activation code adds no global load (its parameters are a kernel argument), so
the tool's allow-list covers these kernels unchanged.  No GPU needed: hipcc cross-compiles (about a minute)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_KERNELS = ("_Z19vjf_mega_act_kernel", "_Z24vjf_mega_lite_act_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc on PATH (the audit tool calls it by name)")
def test_every_plain_load_of_the_act_kernels_is_certified(tmp_path):
    spec = importlib.util.spec_from_file_location("audit_plain_loads", os.path.join(ROOT, "tools", "audit_plain_loads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.KERNELS = ACT_KERNELS
    asm = str(tmp_path / "vjf_abi.s")
    mod.build_asm(asm)
    counts, report, bad = mod.audit(asm)
    assert not bad, "\n".join(bad)
    for k in ACT_KERNELS:
        assert counts[k][0] > 100, (k, counts[k])          # (the kernels are there and their hand-off loads are sc1)
