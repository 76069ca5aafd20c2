"""The dense fills read their record blocks through pointers rebuilt from two v_readlane's (lane_ptr,
assemble_common.hpp).  Rebuilt as generic pointers, every such load is a FLAT load, which counts in lgkmcnt as well as
vmcnt and which the compiler can only wait for with a full drain; lane_ptr therefore hands back a
global (address-space-1) pointer.  No GPU needed: the device assembly of the two files must hold no flat access."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emme_amd", "csrc")
FILES = ["assemble_dense", "assemble_dense_deriv"]


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def test_dense_fills_have_no_flat_memory_access(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "device-asm", "HIPCC=" + hipcc, "KERNELS=" + " ".join(FILES),
                        "ASMDIR=" + str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for f in FILES:
        with open(tmp_path / (f + ".s")) as fh:
            lines = [ln.strip() for ln in fh]
        assert any(ln.startswith("global_load_dwordx4") for ln in lines), f  # (it is the device assembly, with its loads)
        flat = [ln for ln in lines if ln.startswith("flat_load") or ln.startswith("flat_store")]
        assert not flat, (f, len(flat), flat[:4])
