from .audio_preprocessing import (AudioToMelSpectrogramPreprocessor, FilterbankFeatures,  # noqa: F401
                                  SpectrogramAugmentation)
from .conformer_encoder import ConformerEncoder  # noqa: F401
from .squeezeformer_encoder import SqueezeformerEncoder  # noqa: F401
from .conv_asr import ConvASRDecoder  # noqa: F401
from .ctc import CTCLoss  # noqa: F401
from .ctc_decoding import (BeamBatchedCTCDecoder, CTCAligner, CTCBeamStreamState, GreedyCTCDecoder, WER,  # noqa: F401
                           ctc_decoder_from_config, ctc_offsets, word_error_rate)
from .ngram_lm import NGramLM  # noqa: F401
from .boosting_tree import BoostingTree  # noqa: F401
from .rnnt_loss import RNNTLoss, RNNTLossNumba  # noqa: F401
from .tdt_loss import TDTLoss, TDTLossNumba  # noqa: F401
from .rnnt import RNNTDecoder, RNNTJoint  # noqa: F401
from .rnnt_decoding import GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, RNNTDecoding, RNNTWER, Hypothesis  # noqa: F401
from .rnnt_decoding import transducer_fusion_from_config  # noqa: F401
from .confidence import (ConfidenceConfig, ConfidenceMethodConfig, aggregate, confidence_from,  # noqa: F401
                         word_confidence)
