"""wetts_amd -- MI355X (gfx950) native VITS inference behind the WeTTS API.

Python host code + a C-ABI shared library of hand-written HIP kernels (include/wetts_hip.h).
Only what the SynthesizerTrn.infer() hot path needs lives here.
"""
from .config import HParams, get_hparams_from_file, make_config, MODEL_CONFIGS  # noqa: F401
from .models import SynthesizerTrn, load_checkpoint  # noqa: F401
from .discriminators import (DurationDiscriminatorV1, DurationDiscriminatorV2,  # noqa: F401
                             MultiPeriodDiscriminator, MultiPeriodMultiResolutionDiscriminator,
                             WavLMDiscriminator, duration_discriminator_from_hparams,
                             wavlm_discriminator_from_hparams)
from .frontend import (Frontend, FrontendModel, FrontendScores, FrontendSession, HostScores, Model,  # noqa: F401
                       compute_accuracy, prosody_f1)
from .frontend_data import IGNORE_ID, FrontendDataset, VocabTokenizer, collate_fn, read_table  # noqa: F401
from .losses import WavLMLoss  # noqa: F401
from .mel_processing import (mel_spectrogram_torch, posterior_spectrogram, spec_to_mel_torch,  # noqa: F401
                             spectrogram_torch)
from .wavlm import Resample, WavLM, load_wavlm  # noqa: F401


def __getattr__(name):
    # FrontendTrainer on first use: frontend_train is also a `python -m` program, which must not be imported beforehand
    if name == "FrontendTrainer":
        from .frontend_train import FrontendTrainer
        return FrontendTrainer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# (FrontendTrainer is reached through __getattr__ and left out of __all__: a star import must not import frontend_train)
__all__ = ["SynthesizerTrn", "MultiPeriodDiscriminator", "MultiPeriodMultiResolutionDiscriminator",
           "DurationDiscriminatorV1", "DurationDiscriminatorV2", "duration_discriminator_from_hparams",
           "WavLMDiscriminator", "wavlm_discriminator_from_hparams", "WavLMLoss", "WavLM", "Resample", "load_wavlm",
           "FrontendModel", "FrontendSession", "Frontend", "Model", "FrontendScores", "HostScores", "compute_accuracy",
           "prosody_f1", "IGNORE_ID", "FrontendDataset", "VocabTokenizer", "collate_fn", "read_table",
           "load_checkpoint", "HParams", "get_hparams_from_file", "make_config",
           "MODEL_CONFIGS", "spectrogram_torch", "spec_to_mel_torch", "mel_spectrogram_torch", "posterior_spectrogram"]
