"""Confidence estimation for greedy CTC / RNN-T / TDT decoding: the configuration objects of the reference
(`ConfidenceConfig`, `ConfidenceMethodConfig`, parts/utils/asr_confidence_utils.py), the host side of the measures the decoding
kernels compute (`mi355x_ctc_greedy_decode_conf`, `mi355x_*_greedy_decode*_conf`: include/mi355x_asr.h states the formulas) and the
aggregation of token confidences into word confidences.

A measure maps a distribution over V classes to 1 (one-hot) .. 0 (uniform); nothing is clamped.  The kernels take the method as
integers and the constants that depend on (V, alpha) alone -- ln V, V^(1-alpha) and the `b` of the exp-normalised rows -- from
here, computed in double (`ConfidenceMethodConfig.kernel_args`)."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

METHODS = {"max_prob": 0, "gibbs": 1, "tsallis": 2, "renyi": 3}     # MI355X_CONF_*
NORMS = {"lin": 0, "exp": 1}                                        # MI355X_CONF_NORM_*
AGGREGATIONS = {"mean": 0, "min": 1, "max": 2, "prod": 3}           # MI355X_CONF_AGG_*


def _from(cls, cfg, what):
    if cfg is None:
        return cls()
    if isinstance(cfg, cls):
        return cfg
    cfg = dict(cfg)
    unknown = set(cfg) - set(cls.__dataclass_fields__)
    if unknown:
        raise ValueError(f"unknown {what} keys: {sorted(unknown)}")
    return cls(**cfg)


@dataclass
class ConfidenceMethodConfig:
    """name 'max_prob' or 'entropy'; entropy_type 'gibbs' | 'tsallis' | 'renyi', alpha > 0, entropy_norm 'lin' | 'exp' (used by
    'entropy' only).  The defaults are the reference's."""
    name: str = "entropy"
    entropy_type: str = "tsallis"
    alpha: float = 0.33
    entropy_norm: str = "exp"

    def __post_init__(self):
        if self.name not in ("max_prob", "entropy"):
            raise ValueError(f"confidence method name '{self.name}' (known: max_prob, entropy)")
        if self.entropy_type not in ("gibbs", "tsallis", "renyi"):
            raise ValueError(f"entropy_type '{self.entropy_type}' (known: gibbs, tsallis, renyi)")
        if self.entropy_norm not in NORMS:
            raise ValueError(f"entropy_norm '{self.entropy_norm}' (known: lin, exp)")
        self.alpha = float(self.alpha)
        if not self.alpha > 0.0:
            raise ValueError(f"alpha must be > 0, got {self.alpha}")

    @classmethod
    def from_dict(cls, cfg):
        return _from(cls, cfg, "confidence method")

    @property
    def method(self) -> str:
        """the row of the table in use: tsallis / renyi at alpha == 1 exactly are gibbs at alpha = 1.  The kernels receive alpha as
        a float and choose the alpha = 1 row by it, so the row is chosen here by alpha rounded to float as well: an alpha within
        half a float ulp of 1 is alpha = 1 on both sides."""
        if self.name == "max_prob":
            return "max_prob"
        return "gibbs" if ctypes.c_float(self.alpha).value == 1.0 else self.entropy_type

    def constants(self, V: int) -> Tuple[float, float, float]:
        """(k0, k1, k2) = (ln V, V^(1-alpha), b of the exp-normalised gibbs / tsallis row, else 0) in double"""
        if V < 2:
            raise ValueError(f"confidence needs at least 2 classes, got {V}")
        a, m = self.alpha, self.method
        k0, k1, k2 = math.log(V), float(V) ** (1.0 - a), 0.0
        if ctypes.c_float(a).value != 1.0 and self.entropy_norm == "exp":
            if m == "gibbs":
                k2 = math.exp(-a * k1 * k0)
            elif m == "tsallis":
                k2 = math.exp((k1 - 1.0) / (a - 1.0))
        return k0, k1, k2

    def kernel_args(self, V: int):
        """(method, norm, alpha, k0, k1, k2) as the *_conf entry points take them"""
        return (METHODS[self.method], NORMS[self.entropy_norm], self.alpha) + self.constants(V)


@dataclass
class ConfidenceConfig:
    """what to keep (frame / token / word confidence), how frames fold into tokens and tokens into words (`aggregation`; CTC:
    `exclude_blank` = a token's own run of frames, else also the blank frames in front of it), and the measure (`method_cfg`).
    Word confidences are folded from token confidences (and a stream's next chunk appends to them), so a hypothesis carries
    `token_confidence` whenever token OR word confidence is preserved, on the CTC and the transducer paths alike."""
    preserve_frame_confidence: bool = False
    preserve_token_confidence: bool = False
    preserve_word_confidence: bool = False
    exclude_blank: bool = True
    aggregation: str = "min"
    method_cfg: ConfidenceMethodConfig = field(default_factory=ConfidenceMethodConfig)

    def __post_init__(self):
        if self.aggregation not in AGGREGATIONS:
            raise ValueError(f"aggregation '{self.aggregation}' (known: mean, min, max, prod)")
        self.method_cfg = ConfidenceMethodConfig.from_dict(self.method_cfg)

    @classmethod
    def from_dict(cls, cfg):
        return _from(cls, cfg, "confidence")

    @property
    def enabled(self) -> bool:
        return bool(self.preserve_frame_confidence or self.preserve_token_confidence or self.preserve_word_confidence)

    @property
    def wants_tokens(self) -> bool:
        return bool(self.preserve_token_confidence or self.preserve_word_confidence)


def confidence_from(cfg) -> Optional[ConfidenceConfig]:
    """None, a ConfidenceConfig or a plain dict (the `confidence_cfg` key of a `decoding` section) -> ConfidenceConfig, or None
    when nothing is asked for"""
    if cfg is None:
        return None
    cfg = ConfidenceConfig.from_dict(cfg)
    return cfg if cfg.enabled else None


def aggregate(values: Sequence[float], how: str) -> float:
    """mean / min / max / prod of a non-empty list of confidences"""
    if how not in AGGREGATIONS:
        raise ValueError(f"aggregation '{how}' (known: mean, min, max, prod)")
    values = [float(v) for v in values]
    if not values:
        raise ValueError("aggregate: an empty list has no confidence")
    if how == "mean":
        return sum(values) / len(values)
    if how == "min":
        return min(values)
    if how == "max":
        return max(values)
    return math.prod(values)


def word_confidence(tokens: Sequence[str], token_conf: Sequence[float], word_pieces: bool = False, how: str = "min") -> List[float]:
    """one confidence per word of `ctc_offsets(tokens, ...)`: `how` over the token confidences of the word's tokens.  Word pieces: a
    leading U+2581 starts a word.  Characters: the space token separates words and belongs to none."""
    from .ctc_decoding import ctc_offsets
    idx = list(range(len(tokens)))
    # the grouping IS ctc_offsets': with start = end = the token's index a word's offsets name its first and last token
    _, words = ctc_offsets(list(tokens), idx, idx, word_pieces=word_pieces)
    return [aggregate(token_conf[w["start_offset"]: w["end_offset"]], how) for w in words]
