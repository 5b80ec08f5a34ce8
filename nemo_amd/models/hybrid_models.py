"""Drop-in for `nemo.collections.asr.models.EncDecHybridRNNTCTCModel` / `EncDecHybridRNNTCTCBPEModel` (models/
hybrid_rnnt_ctc_models.py, hybrid_rnnt_ctc_bpe_models.py): one encoder, a transducer head (RNN-T or TDT) and an auxiliary CTC head
(`aux_ctc`: a ConvASRDecoder over the encoder output), both trained in one step with
    loss = (1 - ctc_loss_weight) * transducer + ctc_loss_weight * CTC,
and either head decoding (`change_decoding_strategy(decoder_type=...)`, `cur_decoder`).  The class the reference's cache-aware
streaming recipes instantiate: `conformer_stream_step` streams the CTC head like EncDecCTCModel, and the transducer head through
greedy decoding resumed from `previous_hypotheses` (rnnt_models.rnnt_conformer_stream_step, modules/rnnt_decoding.py).  One class
serves characters (`labels`) and SentencePiece (`tokenizer`), as EncDecRNNTModel does.  State-dict keys are the reference's:
`encoder.*`, `decoder.*`, `joint.*`, `ctc_decoder.decoder_layers.0.{weight,bias}`."""
from __future__ import annotations

from typing import Any, Dict

import torch

from ..modules import CTCLoss
from .ctc_models import _build as _build_ctc
from .ctc_models import (_is_beam, ctc_align_audio, ctc_fill_confidence, ctc_transcribe_beam, ctc_transcribe_timestamps,
                         frame_stride_s)
from .rnnt_models import EncDecRNNTModel, fastconformer_tdt_config, fastconformer_transducer_config, rnnt_conformer_stream_step

_GREEDY = ("greedy", "greedy_batch")


def _check_ctc_strategy(dcfg):
    """the auxiliary head's `decoding` section is acceptable (the factory every CTC head shares raises where it is not)"""
    from ..modules import ctc_decoder_from_config
    ctc_decoder_from_config(dcfg, None, what="aux_ctc")


class _CTCHeadText:
    """`rnnt_decoder_predictions_tensor` over the auxiliary CTC head: what `transcribe` / `predict_step` call when
    `cur_decoder == 'ctc'` (encoder output in, hypotheses with `.text` out)"""

    def __init__(self, model):
        self.model = model

    def rnnt_decoder_predictions_tensor(self, encoder_output, encoded_lengths, return_hypotheses=False, partial_hypotheses=None):
        from ..modules.rnnt_decoding import Hypothesis
        if partial_hypotheses is not None:
            raise NotImplementedError("the CTC head streams through `previous_pred_out`, not `partial_hypotheses`")
        m = self.model
        dec = m.ctc_decoding
        log_probs = m.ctc_decoder(encoder_output=encoder_output)
        lens = encoded_lengths.cpu()
        hyps = []
        if _is_beam(dec):   # the best hypothesis of the beam search
            for b, nbest in enumerate(dec.nbest(log_probs, encoded_lengths)):
                ids, score = nbest[0] if nbest else ([], float("-inf"))
                hyps.append(Hypothesis(score=score, y_sequence=torch.tensor(ids, dtype=torch.long), text=dec.ids_to_text(ids),
                                       length=int(lens[b])))
            return hyps
        if dec.confidence_cfg is not None:   # the same decoding with confidences, from the one launch that computes both
            tokens, out_len, score, _, _, fc, tc = (t.cpu() for t in dec.decode_ids_confidence(log_probs, encoded_lengths))
        else:
            tokens, out_len, score = (t.cpu() for t in dec.decode_ids(log_probs, encoded_lengths))
        for b in range(tokens.shape[0]):
            n = int(out_len[b])
            ids = tokens[b, :n].to(torch.long)
            hyps.append(Hypothesis(score=float(score[b]), y_sequence=ids, text=dec.ids_to_text(ids.tolist()), length=int(lens[b])))
            if dec.confidence_cfg is not None:
                ctc_fill_confidence(hyps[-1], dec, ids.tolist(), fc[b, : int(lens[b])].tolist(), tc[b, :n].tolist())
        return hyps


class EncDecHybridRNNTCTCModel(EncDecRNNTModel):
    _takes_aux_ctc = True

    def __init__(self, cfg: Dict[str, Any], trainer=None):
        if not dict(cfg).get("aux_ctc"):
            raise ValueError("The config need to have a section for the CTC decoder named as aux_ctc for Hybrid models.")
        super().__init__(cfg, trainer=trainer)
        aux = dict(self._cfg["aux_ctc"])
        if not aux.get("decoder"):
            raise ValueError("aux_ctc needs a `decoder` section (ConvASRDecoder)")
        dec = dict(aux["decoder"])
        # hybrid_rnnt_ctc_models.py:60-80 / hybrid_rnnt_ctc_bpe_models.py:75-95: the vocabulary of the model goes into the CTC decoder
        vocab = self._cfg.get("labels")
        if vocab is None and self.tokenizer is not None:
            vocab = self.tokenizer.vocab
        if vocab is not None:
            dec["vocabulary"] = list(vocab)
            dec["num_classes"] = len(vocab)
        elif dec.get("num_classes", -1) < 1:
            dec["num_classes"] = self.decoder.blank_idx
        if dec["num_classes"] != self.decoder.blank_idx:
            raise ValueError(f"aux_ctc.decoder.num_classes = {dec['num_classes']}, the transducer head has {self.decoder.blank_idx}")
        if dec.get("feat_in") is None:
            dec["feat_in"] = self.encoder._feat_out
        if not dec.get("feat_in"):
            raise ValueError("param feat_in of the decoder's config is not set!")
        self.ctc_decoder = _build_ctc("decoder", dec)
        self.ctc_loss_weight = float(aux.get("ctc_loss_weight", 0.5))
        if not 0.0 <= self.ctc_loss_weight <= 1.0:
            raise ValueError(f"aux_ctc.ctc_loss_weight must lie in [0, 1]; got {self.ctc_loss_weight}")
        self.ctc_loss = CTCLoss(num_classes=self.ctc_decoder.num_classes_with_blank - 1, zero_infinity=True,
                                reduction=aux.get("ctc_reduction") or "mean_batch")
        _check_ctc_strategy(aux.get("decoding"))
        aux["decoder"] = dec
        self._cfg["aux_ctc"] = aux
        self._ctc_wer = None
        self._parts = {}
        self._validating = False
        self.cur_decoder = "rnnt"

    def trainable_modules(self):
        # backward-completion order is not guaranteed for the two heads; the gradient exchange only needs every module listed
        return [self.encoder, self.decoder, self.joint, self.ctc_decoder]

    # ------------------------------------------------------------------ the CTC head's decoding objects (greedy or beam_batch)
    @property
    def ctc_wer(self):
        """hybrid_rnnt_ctc_models.py:82-95: CTCDecoding + WER over the auxiliary head (`aux_ctc.decoding`: greedy or beam_batch)"""
        if self._ctc_wer is None:
            vocab = getattr(self.ctc_decoder, "vocabulary", None)
            if vocab is None:
                return None
            from ..modules import WER, ctc_decoder_from_config
            self._ctc_wer = WER(ctc_decoder_from_config(self._cfg["aux_ctc"].get("decoding"), list(vocab), what="aux_ctc",
                                                        text_to_ids=self._text_to_ids),
                                use_cer=bool(self._cfg.get("use_cer", False)))
        return self._ctc_wer

    @property
    def ctc_decoding(self):
        wer = self.ctc_wer
        return wer.decoding if wer is not None else None

    def change_decoding_strategy(self, decoding_cfg=None, decoder_type: str = None, verbose: bool = True):
        """hybrid_rnnt_ctc_models.py:330-400: `decoder_type` 'rnnt' (or None) rebuilds the transducer decoding object from
        `decoding_cfg` (kept when None) and makes it the head `transcribe` / `predict_step` / `conformer_stream_step` use; 'ctc'
        does the same for the auxiliary head (`aux_ctc.decoding`)"""
        if decoder_type is None or decoder_type == "rnnt":
            if decoding_cfg is not None:
                strategy = dict(decoding_cfg).get("strategy", "greedy_batch")
                if strategy not in _GREEDY:
                    raise NotImplementedError(f"transducer decoding strategy '{strategy}' (implemented: greedy, greedy_batch)")
                self._cfg["decoding"] = dict(decoding_cfg)
            self._decoding = None
            self._wer = None
            self.cur_decoder = "rnnt"
        elif decoder_type == "ctc":
            if decoding_cfg is not None:
                _check_ctc_strategy(decoding_cfg)
                self._cfg["aux_ctc"]["decoding"] = dict(decoding_cfg)
            self._ctc_wer = None
            self.cur_decoder = "ctc"
        else:
            raise ValueError(f"decoder_type={decoder_type} is not supported. Supported values: [ctc,rnnt]")

    def _text_decoding(self):
        if self.cur_decoder == "ctc":
            return _CTCHeadText(self) if self.ctc_decoding is not None else None
        return self.decoding

    # ------------------------------------------------------------------ timestamps and forced alignment over the CTC head
    @property
    def frame_stride_s(self) -> float:
        return frame_stride_s(self)

    def _ctc_log_probs(self, signal, lengths):
        encoded, enc_len = self.forward(input_signal=signal, input_signal_length=lengths)
        return self.ctc_decoder(encoder_output=encoded), enc_len

    def _ctc_decoding(self):
        return self.ctc_decoding

    def _text_to_ids(self, text: str):
        if self.tokenizer is not None:
            return self.tokenizer.text_to_ids(text)
        from ..data.text import make_parser
        return make_parser(labels=list(self.ctc_decoder.vocabulary), do_normalize=False)(text)

    @torch.no_grad()
    def transcribe(self, audio, batch_size: int = 4, return_hypotheses: bool = False, num_workers: int = 0,
                   channel_selector=None, verbose: bool = False, timestamps: bool = False):
        """EncDecRNNTModel.transcribe; timestamps=True (CTC head selected) returns Hypothesis objects with char / word offsets
        (ctc_models.ctc_transcribe_timestamps).  The transducer head's hypotheses already carry `timestamp` with return_hypotheses."""
        if self.cur_decoder == "ctc" and not timestamps and _is_beam(self.ctc_decoding):   # beam_batch over the CTC head
            return ctc_transcribe_beam(self, audio, batch_size, return_hypotheses, channel_selector)
        if not timestamps:
            return super().transcribe(audio, batch_size, return_hypotheses, num_workers, channel_selector, verbose)
        if self.cur_decoder != "ctc":
            raise NotImplementedError("transcribe(timestamps=True) runs over the CTC head: change_decoding_strategy(decoder_type='ctc')")
        return ctc_transcribe_timestamps(self, audio, batch_size, channel_selector)

    @torch.no_grad()
    def align(self, audio, texts, batch_size: int = 4, channel_selector=None):
        """forced alignment over the auxiliary CTC head, whichever head `cur_decoder` names (ctc_models.ctc_align_audio)"""
        return ctc_align_audio(self, audio, texts, batch_size, channel_selector)

    # ------------------------------------------------------------------ both heads in one step (hybrid_rnnt_ctc_models.py:420-520)
    def _loss_and_wer(self, encoded, encoded_len, decoder, target_length, transcript, transcript_len, compute_wer):
        loss, wer, num, denom = super()._loss_and_wer(encoded, encoded_len, decoder, target_length, transcript, transcript_len,
                                                      compute_wer)
        w = self.ctc_loss_weight
        parts = {"rnnt_loss": loss.detach()}
        if w > 0 or self._validating:   # (training with weight 0 does not run the CTC head at all, as in the reference)
            log_probs = self.ctc_decoder(encoder_output=encoded)
            ctc = self.ctc_loss(log_probs=log_probs, targets=transcript, input_lengths=encoded_len, target_lengths=transcript_len)
            parts["ctc_loss"] = ctc.detach()
            loss = (1 - w) * loss + w * ctc
            if compute_wer and self.ctc_wer is not None:
                self.ctc_wer.update(predictions=log_probs.detach(), predictions_lengths=encoded_len, targets=transcript,
                                    targets_lengths=transcript_len)
                parts["wer_ctc"], parts["wer_ctc_num"], parts["wer_ctc_denom"] = self.ctc_wer.compute()
                self.ctc_wer.reset()
        self._parts = parts
        return loss, wer, num, denom

    def training_step(self, batch, batch_nb=0):
        out = super().training_step(batch, batch_nb)
        parts, logs = self._parts, out["log"]
        self._parts = {}
        logs["train_rnnt_loss"] = parts["rnnt_loss"]
        if "ctc_loss" in parts:
            logs["train_ctc_loss"] = parts["ctc_loss"]
        if "wer_ctc" in parts:
            logs["training_batch_wer_ctc"] = parts["wer_ctc"]
        return out

    @torch.no_grad()
    def validation_pass(self, batch, batch_idx=0, dataloader_idx=0):
        """-> val_loss (the combined loss), val_wer / val_wer_num / val_wer_denom of the transducer head, and the same with `_ctc`
        appended for the auxiliary head"""
        self._validating = True
        try:
            metrics = super().validation_pass(batch, batch_idx, dataloader_idx)
        finally:
            self._validating = False
        parts = self._parts
        self._parts = {}
        if "wer_ctc" in parts:
            metrics.update({"val_wer_num_ctc": parts["wer_ctc_num"], "val_wer_denom_ctc": parts["wer_ctc_denom"],
                            "val_wer_ctc": parts["wer_ctc"]})
        return metrics

    def multi_validation_epoch_end(self, outputs, dataloader_idx: int = 0, prefix: str = "val"):
        res = super().multi_validation_epoch_end(outputs, dataloader_idx, prefix)
        if outputs and f"{prefix}_wer_num_ctc" in outputs[0]:
            num = float(sum(x[f"{prefix}_wer_num_ctc"] for x in outputs))
            denom = float(sum(x[f"{prefix}_wer_denom_ctc"] for x in outputs))
            if self.world_size > 1:
                t = torch.tensor([num, denom], device=res[f"{prefix}_loss"].device, dtype=torch.float64)
                torch.distributed.all_reduce(t)
                num, denom = float(t[0]), float(t[1])
            res["log"][f"{prefix}_wer_ctc"] = num / denom if denom else float("inf")
        return res

    # ------------------------------------------------------------------ cache-aware streaming (parts/mixins/mixins.py:590-700)
    @torch.no_grad()
    def conformer_stream_step(self, processed_signal, processed_signal_length=None, cache_last_channel=None, cache_last_time=None,
                              cache_last_channel_len=None, keep_all_outputs=True, previous_hypotheses=None,
                              previous_pred_out=None, drop_extra_pre_encoded=None, return_transcription=True,
                              return_log_probs=False):
        """one chunk of every stream through the encoder and the head `cur_decoder` names.  'ctc': EncDecCTCModel's step over
        `ctc_decoder` (state in `previous_pred_out`; under `beam_batch` the beam search's in `previous_hypotheses`).  'rnnt':
        rnnt_conformer_stream_step (state in `previous_hypotheses`)."""
        if self.cur_decoder == "ctc":
            return self._ctc_stream_step(self.ctc_decoder, self.ctc_wer, processed_signal, processed_signal_length,
                                         cache_last_channel, cache_last_time, cache_last_channel_len, keep_all_outputs,
                                         previous_pred_out, drop_extra_pre_encoded, return_transcription, return_log_probs,
                                         previous_hypotheses)
        return rnnt_conformer_stream_step(self, processed_signal, processed_signal_length, cache_last_channel, cache_last_time,
                                          cache_last_channel_len, keep_all_outputs, previous_hypotheses, previous_pred_out,
                                          drop_extra_pre_encoded, return_transcription, return_log_probs)

    def change_vocabulary(self, *args, **kwargs):
        raise NotImplementedError("change_vocabulary for the hybrid model (both heads would have to be rebuilt)")

    @classmethod
    def restore_from(cls, restore_path: str, map_location=None, strict: bool = True):
        model = super().restore_from(restore_path, map_location=map_location, strict=strict)
        model.ctc_decoder.weights_updated()
        return model


def fastconformer_hybrid_config(size: str = "large", vocab_size: int = 1024, ctc_loss_weight: float = 0.3, durations=None,
                                streaming: bool = False, att_context_size=None, spec_augment: bool = False,
                                **encoder_overrides) -> Dict[str, Any]:
    """model section of examples/asr/conf/fastconformer/hybrid_transducer_ctc/fastconformer_hybrid_transducer_ctc_bpe.yaml: the
    FastConformer-Transducer model plus `aux_ctc` (ctc_loss_weight 0.3, a ConvASRDecoder on the encoder output, greedy CTC
    decoding); `durations` makes the transducer head a TDT (fastconformer_hybrid_tdt_ctc_bpe.yaml).  `streaming=True` gives the
    encoder of hybrid_cache_aware_streaming/fastconformer_hybrid_transducer_ctc_bpe_streaming.yaml: chunked_limited attention with
    `att_context_size` ([70, 13] = 1.12 s chunks), causal convolutions (LayerNorm in the conv module) and causal down-sampling."""
    if att_context_size is not None and not streaming:
        encoder_overrides["att_context_size"] = list(att_context_size)
    if streaming:
        enc = dict(att_context_size=list(att_context_size or (70, 13)), att_context_style="chunked_limited", conv_context_size="causal",
                   causal_downsampling=True, conv_norm_type="layer_norm")
        enc.update(encoder_overrides)
        encoder_overrides = enc
    if durations:
        cfg = fastconformer_tdt_config(size, vocab_size=vocab_size, durations=durations, spec_augment=spec_augment, **encoder_overrides)
    else:
        cfg = fastconformer_transducer_config(size, vocab_size=vocab_size, spec_augment=spec_augment, **encoder_overrides)
    cfg["aux_ctc"] = dict(ctc_loss_weight=ctc_loss_weight, use_cer=False, ctc_reduction="mean_batch",
                          decoder=dict(_target_="nemo.collections.asr.modules.ConvASRDecoder", feat_in=None, num_classes=vocab_size,
                                       vocabulary=None),
                          decoding=dict(strategy="greedy"))
    return cfg
