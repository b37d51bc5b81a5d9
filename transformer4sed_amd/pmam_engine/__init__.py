"""Forward engine of the PMAM variant (`PaSST_CNN`, src/models/cnn_transformer/passt_cnn.py:9-91).

Reuses every encoder / context-network kernel of the MAT-SED engine and adds, in HIP (csrc/lora.hip, cnn_branch.hip, dw_narrow.hip for
the first two items and the narrow layers' weight gradients, csrc/pmam.hip for the rest):
  * LoRA linears (src/models/lora/layers.py:88-153): the operand image of each encoder weight is W + s B A (one merge kernel per
    weight), so the forward GEMMs are the MAT-SED ones;
  * the CNN branch (src/models/cnn/base.py:62-113): NHWC 16-bit activations, every 3x3 convolution = patch gather + one NT GEMM
    (K = 9 C padded to 64, N = filters padded to 128), BatchNorm folded to a per-channel affine, ContextGating as a second
    GEMM over the channels, gate * dropout * average pooling fused;
  * `attention` frequency pooling (src/models/pooling.py:37-51, 6 heads): k | v projection GEMM + one wave per (frame, head);
  * the 384-wide / 12 x 32-head context network on the 64-wide attention kernels: every head is zero-padded to 64 dims in the
    WEIGHT IMAGES (in_proj / linear_pos rows, out_proj columns, pos_bias_u / v), K and P rows scaled by sqrt(2) so that the
    kernels' 1/8 score scale becomes 1/sqrt(32); the padded dims are exact zeros end to end;
  * the projector merge (passt_cnn.py:57-62) with both projections applied before the interpolations (exact: the interpolation
    weights sum to one), which shrinks the two GEMMs from 1000 to 99 / 250 rows per clip.

`PmamEngine` is one class; its methods live in one module per subsystem (images, cnn, grads, stages), each a plain method-holding base
without state of its own: every attribute is set in `PmamEngine.__init__` below.  geometry.py holds the CNN branch's layer plan, the one
place that decides its shapes, row pitches and kernel routes.
"""
import math

import torch

from ..engine import SedEngine

HD_PAD = 64          # head width the attention kernels are built for
SQRT2 = math.sqrt(2.0)

# (the subsystem modules import the names above from this package: they come after them)
from .geometry import pad128       # noqa: E402,F401
from .images import PmamImages       # noqa: E402
from .cnn import Cnn       # noqa: E402
from .grads import PmamGrads, _LoraSlot       # noqa: E402
from .stages import Stages       # noqa: E402


class PmamEngine(PmamImages, Cnn, PmamGrads, Stages, SedEngine):
    def __init__(self, module):
        super().__init__(module)
        self.lora_skinny = True      # (attribute kept for the kernel tests that exercise the full-dW route)
        self.dec_terms2 = False      # (this context network keeps three split-precision terms in every GEMM)
        self._drop_gen = None
        self._cnn_plans = {}         # (B, T, dw_tn) -> the layer plans of `_cnn_plan`

    def _dropout_generator(self):
        """Seed source of the CNN dropout masks: a generator private to this engine (seeded from torch.initial_seed() on first use), so
        that the process-global CPU generator is advanced only by the draws the reference also makes on it (the augmentation)."""
        if self._drop_gen is None:
            self._drop_gen = torch.Generator()
            self._drop_gen.manual_seed((torch.initial_seed() * 0x9E3779B1 + 0x5ED) % (1 << 63))
        return self._drop_gen

    # ------------------------------------------------------------------ stages of SedEngine.forward (passt_cnn.py:31-88): stages.py
    _mlm_c = True               # the merged sequence is decoder_dim wide
    _embed_stage_always = True  # (ddp.GradReducer's stage order of these models ends with "embed" whenever the stack is walked)

    def _walks_decoder_fwd(self):
        return True     # no heads-only shortcut here: the context network is always walked, forward and backward

    def _walks_decoder(self, G, depth):
        return True

    def _check_forward(self, T, opt, save):
        assert T == 1000
        if opt["rows"] is not None:
            raise NotImplementedError("frequency patchout is not part of the PMAM path")
        if opt["win"] is not None and save:
            raise NotImplementedError("gradient through the sliding-window path is not needed by any PMAM config")
