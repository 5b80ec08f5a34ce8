"""CPU-side checks of the windowed rel-pos flash attention (no kernel is launched): the four C entries refuse bad arguments before
any launch, their names are declared and exported, and ConformerEncoder's path predicate sends a limited context to them only
where the attribute says so."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi355x_relpos_flash_fwd_ctx", "mi355x_relpos_flash_bwd_dq_ctx", "mi355x_relpos_flash_bwd_dkv_ctx",
         "mi355x_relpos_flash_bwd_dpos_ctx"]
P = 0x1000   # dummy aligned pointer the host never dereferences


def _call(name, B=2, H=2, T=40, dk=64, win=(1, 4, 4), req=P, aligned=P, ldq=None):
    """`req`: a required pointer, `aligned`: one whose 16-byte alignment the entry checks (the dK/dV entry checks none)"""
    from nemo_amd._lib import lib
    d = H * dk
    ldq = 3 * d if ldq is None else ldq
    drop = (0, 0, 1.0)
    if name == NAMES[0]:
        a = (aligned, ldq, P, d, P, req, P, P, P, d, P, B, H, T, dk, T, 0.125, *drop, *win, None)
    elif name == NAMES[1]:
        a = (req, P, P, ldq, P, d, P, P, P, P, P, P, aligned, P, 3 * d, None, None, 0, B, H, T, dk, 1 << 40, 0.125, *drop, *win, None)
    elif name == NAMES[2]:
        a = (req, P, P, ldq, P, d, P, P, P, P, P, 3 * d, B, H, T, dk, T, 0.125, *drop, *win, None)
    else:
        a = (req, aligned, P, P, d, None, None, 0, B, H, T, dk, 1 << 40, *win, None)
    return getattr(lib, name)(*a)


BAD = [dict(win=(0, 4, 4)), dict(win=(3, 4, 4)), dict(win=(1, -2, 4)), dict(win=(2, 4, -2)), dict(dk=80), dict(req=0), dict(T=0)]
REFUSALS = [(n, b) for n in NAMES for b in BAD] + [(n, dict(aligned=P + 8)) for n in NAMES if n != NAMES[2]] + \
           [(n, dict(ldq=3 * 128 + 8)) for n in NAMES[:3]]


@pytest.mark.parametrize("name,bad", REFUSALS, ids=lambda x: x if isinstance(x, str) else "-".join(f"{k}={v}" for k, v in x.items()))
def test_entries_refuse_before_any_launch(name, bad):
    assert _call(name, **bad) == 1


def test_names_are_declared_and_exported():
    from nemo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi355x_asr.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(", hdr) and n in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, n)


def _encoder(cdt, **kw):
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    enc = ConformerEncoder(feat_in=80, n_layers=1, d_model=128, n_heads=2, att_context_size=[70, 13],
                           att_context_style="chunked_limited", compute_dtype=cdt, **kw)
    enc._pick_ctx()
    return enc


def test_path_predicate():
    enc = _encoder(torch.bfloat16)
    assert enc.use_flash_ctx_attention is None and enc._ctx == (2, 70, 13) and not enc._flash_ok() and enc._ctx_limited_any()
    assert enc._attn_path(1024, torch.bfloat16, 64) == "gemm" and enc._attn_path(1025, torch.bfloat16, 64) == "flash_ctx"
    enc.use_flash_ctx_attention = True
    assert enc._attn_path(200, torch.bfloat16, 64) == "flash_ctx" and enc._attn_path(200, torch.bfloat16, 128) == "flash_ctx"
    assert enc._attn_path(200, torch.float32, 64) == "gemm" and enc._attn_path(200, torch.bfloat16, 72) == "gemm"
    enc.use_flash_ctx_attention = False
    assert enc._attn_path(200, torch.bfloat16, 64) == "gemm"
    with pytest.raises(ValueError, match="bfloat16"):
        enc._attn_path(1025, torch.bfloat16, 64)


def test_fp32_above_the_limit_names_bf16():
    enc = _encoder(torch.float32)
    with pytest.raises(ValueError, match=r"compute_dtype=torch\.bfloat16"):
        enc._attn_path(1050, torch.float32, 64)
