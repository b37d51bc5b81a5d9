"""Evaluation path right behind the model, by subsystem: codec (`Encoder`, score tables, event decoding),
metrics (weak F1, average precision), ground_truth, psds, event_f1, roc (AUROC, segment-based partial AUROC), evaluator.  Nothing here loads the HIP library before the first launch."""
from .codec import (Encoder, _events_device, _events_frames, _scores_device, _scores_tables, batched_decode_preds,  # noqa: F401
                    check_filter_type, create_score_dataframe, decode_pred_batch_fast, frame_boundaries, read_sed_scores,
                    scaled_median_window, write_sed_scores)
from .evaluator import AudiosetStrongEvaluator, Evaluator, ScoreBufferTuple, _HostStage, remove_extra_events  # noqa: F401
from .event_f1 import (F1_COUNTS, F1_MAX_CLIP_EVENTS, F1_MAX_ESTIMATES, F1_MAX_FRAMES, F1_MAX_SEGMENTS, EventSegmentF1,  # noqa: F401
                       log_sedeval_metrics)
from .ground_truth import _microseconds, _table, build_ground_truth  # noqa: F401
from .metrics import AP_CHUNK, ClassMajorScores, MultilabelAveragePrecision, WeakF1Macro  # noqa: F401
from .roc import (ROC_INTS, MultilabelAUROC, SegmentAUROC, d_prime, get_segment_scores, get_segment_scores_and_overlap_add,  # noqa: F401
                  merge_maestro_ground_truth, merge_overlapping_events, roc_integers, roc_scores, segment_targets, segment_weights)
from .psds import (_PSDS_UNITS, PSDS_BLOCK_CLIPS, PSDS_MAX_CLIP_EVENTS, PSDS_MAX_CT_CLASSES, PSDS_MAX_FRAMES,  # noqa: F401
                   PSDS_PADDED_CLASSES, IntersectionPSDS, compute_psds_from_scores, mean_psds_per_type)
