"""Shared by tests/golden/gen_fusion_golden.py and the fusion-encoder tests: the deterministic
parameters of the gated / cross-attention models (a pure function of seed and state-dict key,
oracle/params.py make_tensor), so the fixtures hold outputs only.

The two gates are moved away from their initial 0.5 and made different from each other, so a
swapped or ignored gate changes every output."""
from collections import OrderedDict

import numpy as np

from oracle.params import make_tensor

# avdino.spec kinds -> oracle.params kinds
_KIND = {"w": "dense_w", "b": "dense_b", "bn_w": "bn_w", "bn_b": "bn_b", "rm": "rm", "rv": "rv",
         "nbt": "nbt", "center": "center"}
GATES = {"gate_image": 0.9, "gate_audio": -0.3}
ENCODERS = {"multi_simple_gated": "GatedMultiModalEncoder",
            "multi_cross_attention": "CrossAttentionMultiModalEncoder"}
# fixture name -> (encoder, training mode); E = D = 32, P = 16, B = 5, G = 2, L = 2, 3 steps
CASES = {"mm_gated_mse_small": ("multi_simple_gated", "mse"),
         "mm_xattn_mse_small": ("multi_cross_attention", "mse"),
         "mm_xattn_default_small": ("multi_cross_attention", "default")}
DIMS = dict(E=32, D=32, P=16, B=5, G=2, L=2)
PSEED, BSEED, STEPS = 611, 6110, 3
# the eval-mode student-feature fixture: two loader batches, the second ragged
EVAL_NAME, EVAL_BATCHES, EVAL_SEED = "xattn_eval_features", (6, 3), 6200


def fusion_spec(mode, E, D, P, encoder):
    from avdino.spec import multimodal_dino_sd
    return multimodal_dino_sd(mode, E, D, P, encoder=encoder)


def fusion_state(spec, seed):
    """key -> ndarray for an avdino.spec state-dict spec."""
    out = OrderedDict()
    for k, (shp, kind) in spec.items():
        if kind == "gate":
            out[k] = np.array(GATES[k.rsplit(".", 1)[1]], np.float32)
        else:
            out[k] = make_tensor(seed, k, shp, _KIND[kind])
    return out
