"""MI355X-native MAT-SED hot path.

Importing this package changes nothing in the process.  One runtime setting is RECOMMENDED to the entry point that owns the process
(bench.py, a training script) and has to be made before HIP initialises: `GPU_MAX_HW_QUEUES=8` (ROCclr's default is 4).  HIP streams are
dealt round-robin onto that many hardware queues; a train step uses three of its own (main, no-grad teacher pass, weight-gradient stream)
and RCCL adds its streams once a process group exists -- with 4 queues the teacher's stream then lands on the main stream's queue and the
two passes serialise (measured at world size 1 with the RCCL path forced on: +2.4 % -> +0.7 % per step with 8 queues,
profiles/r5_host_contention.txt).  `transformer4sed_amd.hostcpu.recommended_env()` returns it for launch scripts; until round 5 the package
set it as an import side effect."""

from .grad_clip import clip_grad_norm_, grad_chunk_table, grad_norms  # noqa: E402,F401  (host arithmetic + lazy imports: loads no library)
from .longform import LongFormDetector, chunk_plan, decode_events, median_filter_long, stitch_scores  # noqa: E402,F401  (likewise)

_TOKENIZER = ("GaussianMixtureTokenizer", "KMeansTokenizer", "FeatureExtractor", "PseudoLabelGenerator", "save_prob")


_EVALUATION = ("IntersectionPSDS", "compute_psds_from_scores", "EventSegmentF1", "log_sedeval_metrics", "MultilabelAUROC", "SegmentAUROC")
_SEARCH = ("PostprocSearch", "PostprocChoice")
_SEBB = ("sebb_bank", "SebbPostprocessor", "SebbSearch", "SebbChoice")
_ENSEMBLE = ("EnsembleSearch", "EnsembleChoice")


def __getattr__(name):      # the PMAM tokenizer (tokenizer.py), the PSDS and the F1 (evaluation/), resolved on first use: they pull in the op layer
    if name in _TOKENIZER:
        from . import tokenizer
        return getattr(tokenizer, name)
    if name in _SEARCH:
        from . import postproc_search
        return getattr(postproc_search, name)
    if name in _SEBB:
        from . import sebb
        return getattr(sebb, name)
    if name in _ENSEMBLE:
        from . import ensemble
        return getattr(ensemble, name)
    if name in _EVALUATION:
        from . import evaluation
        return getattr(evaluation, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
