"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the greedy transducer search with shallow fusion
(mi355x_transducer_greedy_decode with models; include/mi355x_asr.h states the rule), built on tests/stream_decode_oracle.py: its prediction
step and state, its chunking, with every tensor widened to float64.

The models share nothing with the tables the device walks:
  * `DictLM`      the n-gram dict of tests/ctc_beam_lm_oracle.py scored by the recursion of its `cond_logp` (the ARPA definition
                  on tuples) over the values the device holds, each file value times ln 10 rounded to float32;
  * `PhraseBoost` `boost_parts` of tests/ctc_beam_boost_oracle.py: string matching of the phrase set against the stream's labels.
    The increment of a label is boost(y.v) - boost(y) with boost = complete + pending; the returned score keeps `complete` only
    (final term -pending(y)).
`TableModel` is the same interface over NGramLM.lookup / a BoostingTree's tables; tests/test_rnnt_fused_host.py shows that it
gives the hypotheses and scores of the two above.

A model's context is whatever it needs of the stream so far (the tuple of all labels; a table state) and travels in the state
dict under `ctx`, next to the fields of stream_decode_oracle.fresh_state.

One step on frame t, logits z over the V1 labels: mi = arg-max (first maximum); mi == blank: a blank.  Else the label is the first
maximum over v != blank of rank_v = (z[v] - z[mi]) + sum_m alpha_m * look_m(ctx_m, v).  The running score gains
(z[k] - z[mi]) - log sum_v exp(z[v] - z[mi]) + sum_m alpha_m * look_m(ctx_m, k); the score returned adds alpha_m * final_m(ctx_m).
TDT: the duration is the arg-max of the duration logits, everything else as in stream_decode_oracle.decode_chunk.

`decode_chunked_fused` is the free-running chunked search; `forced_walk` walks along given hypotheses and reports per decision
(frame, followed, own, margin, max |logit|), like stream_decode_oracle.tdt_forced_decode_margins."""
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

import ctc_beam_boost_oracle as BO
import ctc_beam_lm_oracle as LO
import stream_decode_oracle as S


def to64(P):
    return {k: v.double() for k, v in P.items()}


class DictLM:
    def __init__(self, ng, order, alpha):
        self.ng, self.order, self.alpha = ng, int(order), float(alpha)

    def start(self):
        return ()

    @staticmethod
    def _value(log10):
        """a value of the file as the device's tables hold it: times ln 10 in float64, that product rounded to float32"""
        return float(np.float32(float(log10) * LO.LN10))

    def _cond(self, ctx, c):
        """`cond_logp` of tests/ctc_beam_lm_oracle.py, the ARPA recursion on tuples, over those values (summed in float64)"""
        g = tuple(ctx) + (c,)
        if g in self.ng:
            return self._value(self.ng[g][0])
        if not ctx:
            raise KeyError(f"label {c} has no unigram")
        return (self._value(self.ng[tuple(ctx)][1]) if tuple(ctx) in self.ng else 0.0) + self._cond(tuple(ctx)[1:], c)

    def look(self, ctx, v):
        return self._cond(LO.context_of(ctx, self.order), int(v))

    def advance(self, ctx, v):
        return tuple(ctx) + (int(v),)

    def final(self, ctx):
        return 0.0


class PhraseBoost:
    def __init__(self, phrases, alpha, cs=1.0, ds=2.0):
        self.phrases, self.alpha, self.cs, self.ds = BO.dedup(phrases), float(alpha), float(cs), float(ds)
        self.labels = {c for p in self.phrases for c in p}
        self._boost = {}

    def _parts(self, y):
        y = tuple(y)
        if y not in self._boost:
            self._boost[y] = BO.boost_parts(self.phrases, y, self.cs, self.ds)
        return self._boost[y]

    def start(self):
        return ()

    def look(self, ctx, v):
        complete, pending = self._parts(ctx)
        if int(v) not in self.labels:   # a label no phrase holds: nothing completes, nothing is pending behind it
            return -pending
        return sum(self._parts(tuple(ctx) + (int(v),))) - (complete + pending)

    def advance(self, ctx, v):
        return tuple(ctx) + (int(v),)

    def final(self, ctx):
        return -self._parts(ctx)[1]


class TableModel:
    """an NGramLM / BoostingTree walked by its own `lookup` (float64 sums of the float32 table values)"""

    def __init__(self, model, alpha):
        self.model, self.alpha = model, float(alpha)

    def start(self):
        return 1

    def look(self, ctx, v):
        return self.model.lookup(ctx, int(v))[0]

    def advance(self, ctx, v):
        return self.model.lookup(ctx, int(v))[1]

    def final(self, ctx):
        fin = getattr(self.model, "state_final", None)
        return float(fin[ctx]) if fin is not None else 0.0


def fresh_state(H: int, blank: int, models, dtype=torch.float64) -> Dict:
    st = S.fresh_state(H, blank)
    st["h"], st["c"] = st["h"].to(dtype), st["c"].to(dtype)
    st["ctx"] = [m.start() for m in models]
    return st


def final_score(state, models, dt=np.float64):
    """the score returned: the running score with alpha_m * final_m added in model order"""
    sc = dt(state["score"])
    for m, c in zip(models, state["ctx"]):
        sc = dt(sc + dt(dt(m.alpha) * dt(m.final(c))))
    return sc


def _label_step(z, V1, blank, models, ctx):
    """-> (mi, k, ranks or None): the arg-max, the label the step takes, and the float64 ranks of a fused step"""
    mi = int(torch.argmax(z[:V1]))
    if mi == blank:
        return mi, blank, None
    ranks = (z[:V1] - z[mi]).clone()
    for m, c in zip(models, ctx):
        if m.alpha != 0.0:
            ranks[:blank] += torch.tensor([m.alpha * m.look(c, v) for v in range(blank)], dtype=ranks.dtype)
    ranks[blank] = -math.inf
    return mi, int(torch.argmax(ranks)), ranks


def _np(t):
    return np.float32 if t.dtype == torch.float32 else np.float64


def _gain(z, V1, mi, k, models, ctx):
    """the gain of the running score in the precision of z, in the rule's association: (((z[k] - z[mi]) - log se) + a_0 l_0) + a_1 l_1"""
    dt = _np(z)
    g = dt(dt(z[k] - z[mi]) - dt(torch.log(torch.exp(z[:V1] - z[mi]).sum())))
    for m, c in zip(models, ctx):
        g = dt(g + dt(dt(m.alpha) * dt(m.look(c, k))))
    return g


def decode_chunk_fused(Pd, Pj, f, state: Dict, blank: int, max_symbols: int, models, durations: Optional[Sequence[int]] = None,
                       changed: Optional[list] = None, gaps: Optional[list] = None):
    """one chunk of one stream (stream_decode_oracle.decode_chunk with the fused rule): f [L, J] -> (tokens, GLOBAL frame
    indices, next state).  `changed` (list) gets (mi, k) appended for every step whose label the models changed; `gaps` the gap
    between the two best ranks of every fused step."""
    _, _, _, _, _, w_out, b_out = S._weights(Pd, Pj)
    L = f.shape[0]
    h, c, last, score, base = state["h"], state["c"], state["last"], state["score"], state["frames_done"]
    skip, same, ctx = state["skip"], state["zero_run"], list(state["ctx"])
    tdt = durations is not None
    V1 = w_out.shape[0] - (len(durations) if tdt else 0)
    assert blank == V1 - 1
    toks, times = [], []
    cap = L * max_symbols if max_symbols else 4 * L
    if L > (skip if tdt else 0):
        gp, hn, cn = S._pred(Pd, Pj, last, h, c)

    def step(t):
        z = F.linear(torch.relu(f[t] + gp), w_out, b_out)
        mi, k, ranks = _label_step(z, V1, blank, models, ctx)
        if ranks is not None:
            if changed is not None and k != mi:
                changed.append((mi, k))
            if gaps is not None:
                top = torch.topk(ranks, 2).values
                gaps.append(float(top[0] - top[1]))
        return z, mi, k

    def emit(z, mi, k, t):
        nonlocal h, c, last, score, gp, hn, cn, ctx
        toks.append(k); times.append(base + t)
        score = _np(z)(score + _gain(z, V1, mi, k, models, ctx))
        ctx = [m.advance(cx, k) for m, cx in zip(models, ctx)]
        h, c, last = hn, cn, k
        gp, hn, cn = S._pred(Pd, Pj, k, h, c)

    if tdt:
        t = skip
        while t < L and len(toks) < cap:
            z, mi, k = step(t)
            d = durations[int(torch.argmax(z[V1:]))]
            if k == blank:
                t += max(d, 1)
                same = 0
            else:
                emit(z, mi, k, t)
                same = same + 1 if d == 0 else 0
                if d == 0 and max_symbols and same >= max_symbols:
                    d, same = 1, 0
                t += d
        skip = max(t - L, 0)
    else:
        for t in range(L):
            sym = 0
            while (sym < max_symbols) if max_symbols else (len(toks) < cap):
                z, mi, k = step(t)
                if k == blank:
                    break
                emit(z, mi, k, t)
                sym += 1
        skip = 0
    nxt = dict(h=h, c=c, last=last, score=score, frames_done=base + L, skip=skip, zero_run=same, ctx=ctx)
    return toks, times, nxt


def decode_chunked_fused(Pd, Pj, f_all, enc_len, blank: int, max_symbols: int, cuts: Sequence[int], models,
                         durations: Optional[Sequence[int]] = None, changed: Optional[list] = None, gaps: Optional[list] = None):
    """the free-running search, every utterance cut at the frame positions `cuts` (as stream_decode_oracle.decode_chunked):
    f_all [B, T, J] float64 -> (list of (tokens, frame indices), list of final states, list of returned scores)"""
    H = Pd["prediction.dec_rnn.lstm.weight_hh_l0"].shape[1]
    T = f_all.shape[1]
    edges = [0] + [int(x) for x in cuts] + [T]
    assert edges == sorted(set(edges)), edges
    hyps, finals, scores = [], [], []
    for b in range(f_all.shape[0]):
        st = fresh_state(H, blank, models, f_all.dtype)
        toks, times = [], []
        n = int(enc_len[b])
        for lo, hi in zip(edges[:-1], edges[1:]):
            L = max(0, min(hi, n) - lo)
            tk, tm, st = decode_chunk_fused(Pd, Pj, f_all[b, lo:lo + L], st, blank, max_symbols, models, durations, changed, gaps)
            toks += tk; times += tm
        hyps.append((toks, times))
        finals.append(st)
        scores.append(final_score(st, models, _np(f_all)))
    return hyps, finals, scores


def forced_walk(Pd, Pj, f_all, enc_len, blank: int, max_symbols: int, models, hyps, durations: Optional[Sequence[int]] = None):
    """Walk the fused search ALONG given hypotheses (list of (tokens, frame indices)).  -> (report, scores): per utterance a list of
    (frame, followed, own, margin, max |logit|) per decision -- followed / own are labels (RNN-T) or (label, duration) (TDT) -- and
    the float64 returned score of the followed hypothesis.  margin = how far this restatement's logits are from taking the followed
    decision, 0 where the two agree:
      own blank, followed a label       z[blank] - max over labels of z (a label has to become the arg-max)
      own a label, followed blank       z[arg-max] - z[blank]
      two labels                        rank[own] - rank[followed]
    TDT: the larger of that and the duration margin, durations followed as in stream_decode_oracle.tdt_forced_decode_margins."""
    _, _, _, _, _, w_out, b_out = S._weights(Pd, Pj)
    H = Pd["prediction.dec_rnn.lstm.weight_hh_l0"].shape[1]
    tdt = durations is not None
    D = len(durations) if tdt else 0
    V1 = w_out.shape[0] - D
    report, scores = [], []
    for b in range(f_all.shape[0]):
        toks, times = list(hyps[b][0]), list(hyps[b][1])
        L = int(enc_len[b])
        h, c = torch.zeros(H, dtype=f_all.dtype), torch.zeros(H, dtype=f_all.dtype)
        gp, hn, cn = S._pred(Pd, Pj, blank, h, c)
        ctx = [m.start() for m in models]
        t, pos, same, sym, score, rows = 0, 0, 0, 0, 0.0, []
        while t < L:
            assert not (pos < len(toks) and times[pos] < t), (b, t, pos, times[pos])
            z = F.linear(torch.relu(f_all[b, t] + gp), w_out, b_out)
            mi, own_k, ranks = _label_step(z, V1, blank, models, ctx)
            on_frame = pos < len(toks) and times[pos] == t
            if not tdt and max_symbols and sym >= max_symbols:   # the frame used up its labels: no decision is taken on it
                assert not on_frame, (b, t)
                t, sym = t + 1, 0
                continue
            k = toks[pos] if on_frame else blank
            if own_k == k:
                margin = 0.0
            elif own_k == blank:
                margin = float(z[blank] - z[:blank].max())
            elif k == blank:
                margin = float(z[mi] - z[blank])
            else:
                margin = float(ranks[own_k] - ranks[k])
            if not tdt:
                rows.append((t, k, own_k, margin, float(z.abs().max())))
                if k == blank:
                    t, sym = t + 1, 0
                    continue
            else:
                own_i = int(torch.argmax(z[V1:]))
                nxt_pos = pos + 1 if on_frame else pos
                limit = times[nxt_pos] if nxt_pos < len(toks) else None

                def step_of(i):
                    d = durations[i]
                    if k == blank:
                        return max(d, 1)
                    if d == 0 and max_symbols and same + 1 >= max_symbols:
                        return 1
                    return d
                ok = [i for i in range(D) if limit is None or t + step_of(i) <= limit]
                assert ok, (b, t, pos)
                fol_i = own_i if own_i in ok else max(ok, key=lambda i: (float(z[V1 + i]), -i))
                margin = max(margin, float(z[V1 + own_i] - z[V1 + fol_i]))
                rows.append((t, (k, durations[fol_i]), (own_k, durations[own_i]), margin, float(z.abs().max())))
                d = durations[fol_i]
                if k == blank:
                    t += max(d, 1)
                    same = 0
                    continue
            # the followed label is emitted: its own arg-max reference if the device's arg-max was a label (the step's gain is
            # defined relative to lg[mi]; where this side's arg-max is the blank the device's was a label within the margin)
            ref = mi if mi != blank else int(torch.argmax(z[:blank]))
            score = _np(z)(score + _gain(z, V1, ref, k, models, ctx))
            ctx = [m.advance(cx, k) for m, cx in zip(models, ctx)]
            pos += 1
            h, c = hn, cn
            gp, hn, cn = S._pred(Pd, Pj, k, h, c)
            if tdt:
                same = same + 1 if d == 0 else 0
                if d == 0 and max_symbols and same >= max_symbols:
                    d, same = 1, 0
                t += d
            else:
                sym += 1
        assert pos == len(toks), (b, pos, len(toks))
        report.append(rows)
        scores.append(final_score(dict(score=score, ctx=ctx), models, _np(f_all)))
    return report, scores


# ---- the models of the GPU cases (tests/test_rnnt_fused_host.py asserts their input conditions on the CPU)
TREE_ALPHA, LM_ALPHA, MAX_SYMBOLS, LM_SEED, LM_ORDER = 2.0, 0.5, 5, 3, 3


def phrases_from(hyps, V, seed=0):
    """key phrases taken from the unfused hypotheses themselves (random phrases would never be spelled): runs of 2-3 labels, and a
    sibling of each that differs in the last label, so that phrases are begun, completed, failed and left pending"""
    g = torch.Generator().manual_seed(1234 + seed)
    out = []
    for toks, _ in hyps:
        for _ in range(3):
            if len(toks) < 3:
                continue
            n = int(torch.randint(2, 4, (1,), generator=g))
            i = int(torch.randint(0, len(toks) - n + 1, (1,), generator=g))
            p = tuple(int(x) for x in toks[i:i + n])
            out.append(p)
            out.append(p[:-1] + ((p[-1] + 1 + int(torch.randint(0, V - 1, (1,), generator=g))) % V,))
    return BO.dedup(out)


DUR = [0, 1, 2, 3, 4]
WIDE = dict(V=1100, H=32, D=24, J=32, T=12, lens=[12, 10])   # V1 = 1101: three strides of the 512-thread pass, the last partial
# (the blank has to beat the largest of 1100 label logits now and then: at + 11 the RNN-T case has frames with 0, 3 and 5 labels,
# at + 12 the TDT case 5 blank decisions among its 41)
WIDE_SEED, WIDE_BLANK_BIAS = 7, dict(rnnt=11.0, tdt=12.0)
_cases = {}


def table_lm(ng, V):
    """the NGramLM the loader builds from the dict's ARPA text"""
    import os
    import tempfile
    from nemo_amd.modules.ngram_lm import NGramLM
    with tempfile.TemporaryDirectory() as d:
        LO.write_arpa(ng, os.path.join(d, "lm.arpa"))
        return NGramLM.from_arpa(os.path.join(d, "lm.arpa"), V)


def fused_case(kind: str, shape: str = "small"):
    """everything the tests share about one case, computed once: dict(Pd, Pj: fp32 state-dicts, Pd64, Pj64, enc, f_all (fp32
    [B, T, J]), lens, V, durations, max_symbols, base: the unfused hypotheses, phrases, ng).  `small`: SMALL of
    stream_decode_oracle with its RNN-T / TDT settings; `wide`: V = 1100."""
    key = (kind, shape)
    if key not in _cases:
        durations = DUR if kind == "tdt" else None
        if shape == "small":
            V, lens = S.SMALL["V"], torch.tensor(S.SMALL["lens"])
            Pd, Pj = S.small_case(kind)
            enc = S.small_enc()
        else:
            V, H, D, J, T = (WIDE[k] for k in "VHDJT")
            lens = torch.tensor(WIDE["lens"])
            Pd, Pj = S.random_transducer(WIDE_SEED, V, H, D, J, n_dur=5 if kind == "tdt" else 0, scale=4.0,
                                         blank_bias=WIDE_BLANK_BIAS[kind], dur0_bias=1.0 if kind == "tdt" else 0.0)
            enc = torch.randn(len(lens), D, T, generator=torch.Generator().manual_seed(107)) * 1.5
        f_all = F.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"]).contiguous()
        Pd64, Pj64 = to64(Pd), to64(Pj)
        base, _, _ = decode_chunked_fused(Pd64, Pj64, f_all.double(), lens, V, MAX_SYMBOLS, [], [], durations)
        _cases[key] = dict(Pd=Pd, Pj=Pj, Pd64=Pd64, Pj64=Pj64, enc=enc, f_all=f_all, lens=lens, V=V, durations=durations,
                           max_symbols=MAX_SYMBOLS, base=base, phrases=phrases_from(base, V), ng=LO.make_lm(LM_SEED, V, LM_ORDER))
    return _cases[key]


def case_models(case, which: str, tables: bool = False, tree_alpha: float = TREE_ALPHA, lm_alpha: float = LM_ALPHA):
    """the oracle models of `which` in ('tree', 'lm', 'both'), the LM first as the decoding objects order them; tables=True: the
    same over the NGramLM / BoostingTree tables -> (oracle models, [(NGramLM | BoostingTree, alpha)] for the op)"""
    from nemo_amd.modules.boosting_tree import BoostingTree
    V = case["V"]
    if "tables" not in case:
        case["tables"] = dict(lm=table_lm(case["ng"], V), tree=BoostingTree.from_phrases(case["phrases"], V))
    want = [w for w in ("lm", "tree") if which in (w, "both")]
    alpha = dict(lm=lm_alpha, tree=tree_alpha)
    pairs = [(case["tables"][w], alpha[w]) for w in want]
    if tables:
        return [TableModel(m, a) for m, a in pairs], pairs
    plain = dict(lm=lambda: DictLM(case["ng"], LM_ORDER, lm_alpha), tree=lambda: PhraseBoost(case["phrases"], tree_alpha))
    return [plain[w]() for w in want], pairs
