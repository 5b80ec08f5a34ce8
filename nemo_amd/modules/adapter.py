"""Linear adapters (the reference's `LinearAdapter` and `adapter_mixins`): a bottleneck MLP behind a LayerNorm added to the residual
stream of every Conformer layer, so that a pretrained model is fine-tuned with its own weights frozen and only the adapter trained
and shipped.  The arithmetic is one fused kernel per direction (csrc/adapter.hip); the rule is stated in include/mi355x_asr.h.

`LinearAdapter` holds the reference's parameter layout only (`module.0` LayerNorm, `module.1.weight` [dim, d], `module.3.weight`
[d, dim], zero-initialised); `AdapterHost` is what ConformerEncoder mixes in, `AdapterModelMixin` what the models forward to it."""
from __future__ import annotations

import torch
from torch import nn

from .. import ops

MAX_D = 1024   # the kernel's limit on in_features (include/mi355x_asr.h)


def read_config(cfg, d, compute_dtype=torch.bfloat16):
    """-> dim of a `LinearAdapter` config (dict or keyword-style object) for in_features = d; everything the kernel does not compute is
    refused by name (the kernel reads 16-byte weight vectors: d in steps of 8 for bf16 compute, of 4 for fp32)"""
    cfg = dict(cfg)
    target = str(cfg.get("_target_", "LinearAdapter"))
    if not target.endswith("LinearAdapter"):
        raise NotImplementedError(f"adapter {target}: only LinearAdapter is implemented")
    if int(cfg.get("in_features", d)) != d:
        raise ValueError(f"adapter in_features={cfg.get('in_features')} but the encoder's d_model is {d}")
    bad = []
    if cfg.get("norm_position", "pre") != "pre": bad.append(f"norm_position: {cfg['norm_position']}")
    if float(cfg.get("dropout", 0.0)) > 0.0: bad.append("dropout > 0")
    if cfg.get("activation", "swish") != "swish": bad.append(f"activation: {cfg['activation']} (implemented: swish)")
    st = dict(cfg.get("adapter_strategy") or {})
    if float(st.get("stochastic_depth", 0.0)) > 0.0: bad.append("stochastic_depth > 0")
    if float(st.get("l2_lambda", 0.0)) > 0.0: bad.append("l2_lambda > 0")
    dim = int(cfg.get("dim", 0))
    if dim < 8 or dim > 128 or dim % 8: bad.append(f"dim={dim} (implemented: the multiples of 8 in 8..128)")
    step = 4 if compute_dtype == torch.float32 else 8
    if d > MAX_D: bad.append(f"d={d} above the kernel's limit ({MAX_D})")
    if d % step: bad.append(f"d={d} is not a multiple of {step} (4 only with compute_dtype=torch.float32)")
    if bad:
        raise NotImplementedError("MI355X LinearAdapter does not implement: " + ", ".join(bad))
    return dim


class LinearAdapter(nn.Module):
    def __init__(self, in_features, dim, **cfg):
        super().__init__()
        self.cfg = dict(cfg, in_features=in_features, dim=dim)
        self.dim = read_config(self.cfg, in_features)
        up = nn.Linear(dim, in_features, bias=False)
        nn.init.zeros_(up.weight)
        self.module = nn.Sequential(nn.LayerNorm(in_features), nn.Linear(in_features, dim, bias=False), nn.SiLU(), up)
        self.enabled = True

    norm = property(lambda self: self.module[0])
    down = property(lambda self: self.module[1])
    up = property(lambda self: self.module[3])


def split_name(name, module="encoder"):
    """'name' or 'encoder:name' -> name; adapters on other modules ('decoder:...', 'joint:...') are refused"""
    if ":" in name:
        where, name = name.split(":", 1)
        if where != module:
            raise NotImplementedError(f"adapters on '{where}' ({where}:{name}): only the Conformer encoder takes adapters")
    return name


class AdapterHost:
    """adapter bookkeeping and launches of ConformerEncoder: adapters live at layers.{i}.adapter_layer.{name}"""
    adapters_supported = True

    def _adapter_names(self):
        al = getattr(self.layers[0], "adapter_layer", None)
        return list(al.keys()) if al is not None else []

    def _enabled_adapters(self, L):
        al = getattr(L, "adapter_layer", None)
        return [(n, a) for n, a in al.items() if a.enabled] if al is not None else []

    def is_adapter_available(self):
        return bool(self._adapter_names())

    def add_adapter(self, name, cfg):
        if not self.adapters_supported:
            raise NotImplementedError(f"adapters on {type(self).__name__}: only ConformerEncoder takes adapters")
        name = split_name(name)
        dim = read_config(cfg, self.d_model, self.compute_dtype)
        if name in self._adapter_names():
            raise ValueError(f"adapter '{name}' already exists")
        kw = {k: v for k, v in dict(cfg).items() if k not in ("_target_", "in_features", "dim")}
        dev = next(self.parameters()).device
        for L in self.layers:
            if getattr(L, "adapter_layer", None) is None:
                L.adapter_layer = nn.ModuleDict()
            L.adapter_layer[name] = LinearAdapter(self.d_model, dim, **kw).to(dev)
        self._flatp.build(dev)       # new parameters: new flat storage, `generation` bumps and with it image plans and optimizer state
        self._adapters_changed()

    def set_enabled_adapters(self, name=None, enabled=True):
        if not self.is_adapter_available():
            raise ValueError("no adapter has been added")
        name = split_name(name) if name is not None else None
        if name is not None and name not in self._adapter_names():
            raise ValueError(f"adapter '{name}' does not exist (have: {self._adapter_names()})")
        for L in self.layers:
            for n, a in L.adapter_layer.items():
                if name is None or n == name:
                    a.enabled = bool(enabled)
        self._adapters_changed()

    def get_enabled_adapters(self):
        return [n for n, _ in self._enabled_adapters(self.layers[0])]

    def unfreeze_enabled_adapters(self):
        for L in self.layers:
            for _, a in self._enabled_adapters(L):
                a.train()
                for p in a.parameters():
                    p.requires_grad = True

    def _adapters_changed(self):
        """another set of launches from now on: recorded launch tapes and graph decisions belong to the old one"""
        self._graph_sets.clear()
        self._cur_gs = None

    def adapter_state(self, name=None):
        """{'state_dict': the adapters' entries of the state-dict, 'configs': {name: cfg}}"""
        names = self._adapter_names() if name is None else [split_name(name)]
        for n in names:
            if n not in self._adapter_names():
                raise ValueError(f"adapter '{n}' does not exist (have: {self._adapter_names()})")
        sd = {k: v.detach().clone() for k, v in self.state_dict().items()
              if ".adapter_layer." in k and k.split(".adapter_layer.")[1].split(".")[0] in names}
        return {"state_dict": sd, "configs": {n: dict(self.layers[0].adapter_layer[n].cfg) for n in names}}

    def load_adapter_state(self, state, name=None):
        if name is not None and split_name(name) not in state["configs"]:
            raise ValueError(f"adapter '{split_name(name)}' is not in the file (it holds: {list(state['configs'])})")
        for n, cfg in state["configs"].items():
            if name is not None and n != split_name(name):
                continue
            if n not in self._adapter_names():
                self.add_adapter(n, cfg)
            own = dict(self.named_parameters())
            with torch.no_grad():
                for k, v in state["state_dict"].items():
                    if k.split(".adapter_layer.")[1].split(".")[0] == n:
                        own[k].copy_(v)
        self.weights_updated()

    # ------------------------------------------------------------------ images and launches
    def _declare_adapter_images(self, p):
        for i, L in enumerate(self.layers):
            al = getattr(L, "adapter_layer", None)
            for n, a in (al.items() if al is not None else ()):
                p.add_matrix(f"L{i}.ad.{n}.wd", a.down.weight.data); p.add_matrix(f"L{i}.ad.{n}.wdt", a.down.weight.data, True)
                p.add_matrix(f"L{i}.ad.{n}.wu", a.up.weight.data); p.add_matrix(f"L{i}.ad.{n}.wut", a.up.weight.data, True)

    def _adapters_fwd(self, i, L, r, W, M):
        """the enabled adapters of layer i on the rows r [M, d] -> (adapted rows, [(adapter, its image prefix, its input)])"""
        saved = []
        for n, a in self._enabled_adapters(L):
            pfx, d = f"L{i}.ad.{n}", self.d_model
            y = self._new(M, d, dtype=torch.float32, device=r.device)
            ops.adapter_fwd(r, a.norm.weight, a.norm.bias, W[pfx + ".wd"], W[pfx + ".wu"], y, M, d, a.dim, a.norm.eps,
                            ld_down=W.pitch(pfx + ".wd"), ld_up=W.pitch(pfx + ".wu"))
            saved.append((a, pfx, r))
            r = y
        return r, saved

    def _adapters_bwd(self, saved, dr, W, M):
        d = self.d_model
        for a, pfx, x in reversed(saved):
            nbytes = ops.adapter_workspace_bytes(M, d, a.dim, W[pfx + ".wd"].dtype)
            ws = self._new((nbytes + 3) // 4, dtype=torch.float32, device=dr.device)
            dx = self._new(M, d, dtype=torch.float32, device=dr.device)
            ops.adapter_bwd(x, dr, a.norm.weight, a.norm.bias, W[pfx + ".wd"], W[pfx + ".wut"], W[pfx + ".wdt"], dx, a.down.weight.grad,
                            a.up.weight.grad, a.norm.weight.grad, a.norm.bias.grad, ws, M, d, a.dim, a.norm.eps,
                            ld_down=W.pitch(pfx + ".wd"), ld_up_t=W.pitch(pfx + ".wut"), ld_down_t=W.pitch(pfx + ".wdt"))
            dr = dx
        return dr


class AdapterModelMixin:
    """the adapter interface of the models: forwarded to `self.encoder`"""

    def add_adapter(self, name, cfg):
        self.encoder.add_adapter(split_name(name), cfg)

    def is_adapter_available(self):
        return self.encoder.is_adapter_available()

    def set_enabled_adapters(self, name=None, enabled=True):
        self.encoder.set_enabled_adapters(name, enabled)

    def get_enabled_adapters(self):
        return self.encoder.get_enabled_adapters()

    def unfreeze_enabled_adapters(self):
        self.encoder.unfreeze_enabled_adapters()

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def unfreeze(self):
        for p in self.parameters():
            p.requires_grad = True
        self.train()

    def save_adapters(self, path, name=None):
        torch.save(self.encoder.adapter_state(name), path)

    def load_adapters(self, path, name=None):
        self.encoder.load_adapter_state(torch.load(path, map_location="cpu"), name)
