"""What every module that sequences its own forward and backward over libmi355x_asr.so keeps underneath (ConformerEncoder and
SqueezeformerEncoder, ConvASRDecoder, RNNTDecoder, RNNTJoint): flat parameter storage, the compute-dtype rule, the token tensor that
hangs the module's one autograd node on the graph, and the cache of packed GEMM-operand images (nemo_amd/packing.py) that is packed
again when the weights moved.  The image plan has a pure half and a launching half, like the GEMM plan: `_declare_images` /
`_build_plan` only describe the images (they work on the CPU, tests/test_engine_host.py pins them), `_plan` runs the pack.

Also here, once: the output-tile count and the split-K chooser of the atomic weight-gradient GEMMs, and the plain TN weight-gradient
launch of the heads."""
from __future__ import annotations

import torch

from .. import ops
from ..core import NeuralModule
from ..flat import FlatParams
from ..packing import PackPlan


def tiles(n_out, n_in, bf16):
    """output tiles of a [n_out, n_in] weight gradient: 256 x 128 in bf16, 64 x 64 in fp32"""
    return ((n_out + 255) // 256) * ((n_in + 127) // 128) if bf16 else ((n_out + 63) // 64) * ((n_in + 63) // 64)


def splitk(tiles, K, strided_c=False, cap=16):
    """split-K factor for `tiles` output tiles: the factor (<= 16, at least 16 K-tiles per workgroup) whose workgroup
    count fills whole rounds of the 256 CUs best, smaller factors preferred (every extra slice is one more atomic
    pass over the output)"""
    nk = (K + 63) // 64
    if strided_c:
        # atomics into a column-strided C (reference weight layouts) are expensive: only fill the chip once, >= 4 K-tiles per slice.
        # Also the rule of the heads' plain weight gradients (`wgrad_tn`); `cap` = None (ConvASRDecoder) lifts the limit of 16
        # slices, which matters below 16 tiles (1 tile, 8032 rows: 31 slices instead of 16)
        sk = min(nk // 4 if nk >= 8 else 1, 256 // max(tiles, 1))
        return max(1, sk if cap is None else min(sk, cap))
    if tiles < 16:
        # skinny problems (e.g. the [C, C] pointwise-conv weight gradients of 'dw_striding' over 320 000 positions: 2 tiles):
        # 16 slices would leave them on 32 CUs (measured: 9.5 ms for 42 GFLOP); one round of the chip, >= 16 K-tiles each
        return max(1, min(256 // max(tiles, 1), nk // 16, 128))
    best, best_score = 1, -1.0
    for c in range(1, 17):
        if c > 1 and nk // c < 16:
            break
        blocks = tiles * c
        eff = blocks / (((blocks + 255) // 256) * 256)
        score = eff - 0.01 * c
        if score > best_score + 1e-9:
            best, best_score = c, score
    return best


def wgrad_tn(dY, ldy, X, ldx, dW, n_out, n_in, rows, bias_grad=None, cap=16):
    """dW[n_out, n_in] += dY^T @ X (atomic split-K TN GEMM); bias_grad += column sums of dY (a launch of its own)"""
    if bias_grad is not None:
        ops.colsum(dY, bias_grad, rows, n_out, ld=ldy)
    sk = splitk(tiles(n_out, n_in, dY.dtype == torch.bfloat16), rows, strided_c=True, cap=cap)
    ops.gemm(dY, X, dW, n_out, n_in, rows, ldy, ldx, n_in, transA=True, transB=True, atomic=True, splitk=sk, c_dtype=ops.F32)


def declare_padded_heads(p, pf, prefix, attn, d, H, dk, dkp, dA):
    """the eight attention images of one layer with zero-padded heads (see ConformerEncoder._geometry): head h = rows / columns
    h*dkp .. h*dkp + dk of `prefix`.wqkv / wqkvt / wpos / wo / wot in `p` and of the bias rows bqkv / bu / bv in `pf`"""
    qkv = [attn.linear_q.weight.data, attn.linear_k.weight.data, attn.linear_v.weight.data]
    wpos, wo = attn.linear_pos.weight.data, attn.linear_out.weight.data  # wo [d, H*dk]
    p.new_image(f"{prefix}.wqkv", 3 * dA, d); p.new_image(f"{prefix}.wqkvt", d, 3 * dA)
    p.new_image(f"{prefix}.wpos", dA, d)
    p.new_image(f"{prefix}.wo", d, dA); p.new_image(f"{prefix}.wot", dA, d)
    pf.new_image(f"{prefix}.bqkv", 1, 3 * dA)
    pf.new_image(f"{prefix}.bu", 1, dA); pf.new_image(f"{prefix}.bv", 1, dA)
    for h in range(H):
        for j, w in enumerate(qkv):
            p.add_block(f"{prefix}.wqkv", w.view(-1)[h * dk * d:], dk, d, row_off=j * dA + h * dkp, sr1=d, sc1=1)
            p.add_block(f"{prefix}.wqkvt", w.view(-1)[h * dk * d:], d, dk, col_off=j * dA + h * dkp, sr1=1, sc1=d)
        p.add_block(f"{prefix}.wpos", wpos.view(-1)[h * dk * d:], dk, d, row_off=h * dkp, sr1=d, sc1=1)
        p.add_block(f"{prefix}.wo", wo.view(-1)[h * dk:], d, dk, col_off=h * dkp, sr1=d, sc1=1)
        p.add_block(f"{prefix}.wot", wo.view(-1)[h * dk:], dk, d, row_off=h * dkp, sr1=1, sc1=d)
        for j, b in enumerate((attn.linear_q.bias.data, attn.linear_k.bias.data, attn.linear_v.bias.data)):
            pf.add_block(f"{prefix}.bqkv", b[h * dk:], 1, dk, col_off=j * dA + h * dkp, sr1=0, sc1=1)
        pf.add_block(f"{prefix}.bu", attn.pos_bias_u.data.view(-1)[h * dk:], 1, dk, col_off=h * dkp, sr1=0, sc1=1)
        pf.add_block(f"{prefix}.bv", attn.pos_bias_v.data.view(-1)[h * dk:], 1, dk, col_off=h * dkp, sr1=0, sc1=1)


class EngineModule(NeuralModule):
    def _init_engine(self, compute_dtype, tail=None):
        """engine state (not part of the state-dict); `tail`: see FlatParams"""
        self.compute_dtype = compute_dtype  # None: bf16 under torch autocast(bf16), else fp32
        self.grad_ready_hook = None  # callable(start, end) on the flat gradient buffer (data-parallel bucketing)
        self._flatp = FlatParams(self, tail=tail)
        self._plans = {}
        self._weights_version = -1
        self._token = None
        self._step_seed = 0
        self._force_pack = False    # run the weight-image pack at every _plan call (a recorded forward always re-packs)

    def flat_parameters(self) -> FlatParams:
        self._flatp.ensure()
        return self._flatp

    def weights_updated(self):
        """call after an optimizer step / load_state_dict: GEMM operand images are re-packed on next forward"""
        self._weights_version += 1

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.weights_updated()
        return r

    def _cdt(self):
        if self.compute_dtype is not None:
            return self.compute_dtype
        if torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() == torch.bfloat16:
            return torch.bfloat16
        return torch.float32

    def _tok(self, device):
        if self._token is None or self._token.device != device:
            self._token = torch.zeros(1, device=device, requires_grad=True)
        return self._token

    # ------------------------------------------------------------------ packed weight images
    def _declare_images(self, p, pf):
        """declarations only: GEMM-operand images in `p` (compute dtype), fp32 bias images in `pf`"""
        raise NotImplementedError

    def _plan_key(self, cdt, device):
        return (cdt, str(device), self._flatp.generation)

    def _build_plan(self, cdt, device):
        """-> (W, Wf): the finalized image plans, Wf None when nothing was declared in fp32.  Launches nothing."""
        p, pf = PackPlan(cdt, device), PackPlan(torch.float32, device)
        self._declare_images(p, pf)
        p.finalize()
        if not pf._images:
            return p, None
        pf.finalize()
        return p, pf

    def _plan(self, cdt, device):
        """-> (W, Wf) holding the current weights"""
        key = self._plan_key(cdt, device)
        entry = self._plans.get(key)
        if entry is None:
            self._plans = {}  # parameters moved: drop images of the old storage
            entry = self._plans[key] = [self._build_plan(cdt, device), -2]
        if entry[1] != self._weights_version or self._force_pack:
            for plan in entry[0]:
                if plan is not None:
                    plan.run()
            entry[1] = self._weights_version
        return entry[0]
