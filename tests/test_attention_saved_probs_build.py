"""Build checks of the saved-probabilities attention kernels (no GPU): hipcc cross-compiles nemo_amd/csrc/attention.hip for gfx950
and reports every kernel's resources.

  * neither given-P instantiation (dQ, dK/dV) nor the exporting forward uses scratch memory;
  * dQ with given probabilities needs fewer vector registers than the recomputing dQ kernel's 256;
  * the forward, with and without the export, stays at <= 168 VGPRs (512 / 3: a third workgroup per CU stays possible);
  * tools/check_asm_loads.py accepts the assembly (no register of an inline-asm load is touched before its wait).
"""
import functools
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not found")


@functools.lru_cache(maxsize=None)
def compiled(tmp):
    from nemo_amd.build import FLAGS
    asm = os.path.join(tmp, "attention.s")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc"] + FLAGS + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                       os.path.join(ROOT, "nemo_amd", "csrc", "attention.hip"), "-o", asm], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    res = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", r.stderr, re.S):
        res[m.group(1)] = dict(vgprs=int(m.group(2)), scratch=int(m.group(3)), lds=int(m.group(4)))
    return asm, res


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    return compiled(str(tmp_path_factory.mktemp("attn_asm")))


def kernel(res, name, dk, flag):
    hits = [v for k, v in res.items() if re.match(rf"_Z\d+{name}ILi{dk}ELb{flag}E", k)]
    assert len(hits) == 1, (name, dk, flag, sorted(res))
    return hits[0]


def test_given_p_kernels_use_no_scratch_and_fewer_registers(build):
    _, res = build
    fwd, fwd_p = kernel(res, "relpos_flash_fwd_kernel", 64, 0), kernel(res, "relpos_flash_fwd_kernel", 64, 1)
    dq, dq_p = kernel(res, "relpos_flash_bwd_dq_kernel", 64, 0), kernel(res, "relpos_flash_bwd_dq_kernel", 64, 1)
    dkv_p = kernel(res, "relpos_flash_bwd_dkv_kernel", 64, 1)
    print(dict(fwd=fwd, fwd_p=fwd_p, dq=dq, dq_p=dq_p, dkv_p=dkv_p))
    assert fwd_p["scratch"] == 0 and dq_p["scratch"] == 0 and dkv_p["scratch"] == 0
    assert dq_p["vgprs"] < 256 and dq_p["vgprs"] < dq["vgprs"]
    assert fwd["vgprs"] <= 168 and fwd_p["vgprs"] <= 168
    # two workgroups per CU (160 KiB of LDS): every kernel of the d_k = 64 family at <= 80 KiB
    assert max(fwd_p["lds"], dq_p["lds"], dkv_p["lds"]) <= 80 * 1024
    # only head width 64 has the variants
    assert not [k for k in res if re.search(r"ILi128ELb1E", k)]


def test_inline_asm_loads_are_not_touched_before_their_wait(build):
    asm, _ = build
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_loads.py"), asm], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
