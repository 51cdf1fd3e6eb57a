"""Architecture tables of the reference's hot-path models and their state-dict layout.

Names, shapes and order reproduce the reference's ``state_dict`` keys exactly so that
checkpoints interoperate:
  CentralUnimodalImage/Audio      reference models/unimodal.py:105-221
  image_encoder / audio_encoder   models/dino.py:18-73
  CentralMultiModalEncoder        models/dino.py:454-468 (fusion: 214-234)
  SimpleMultiModalEncoder         models/dino.py:214-234 (image_encoder / audio_encoder, 18-73)
  GatedMultiModalEncoder          models/dino.py:237-259 (gate_image / gate_audio)
  CrossAttentionMultiModalEncoder models/dino.py:407-452 (CrossModalAttention 385-404)
  ProjectionHead                  models/dino.py:1240-1254
  MultiModalDINO*                 models/dino.py:588-632, 964-970, 1053-1058, 1156-1161
  UniModalDINO / ImageEncoder     models/dino.py:1257-1297, 483-499
  SpectrogramEncoder              models/dino.py:502-513
  MultiModalSimCLRModel           other_ssl/multimodal_simclr/multimodal_simclr.py:12-20
"""
from collections import OrderedDict


class ConvStackSpec:
    """[conv(K, pad) -> BN2d -> ReLU -> maxpool2] x L (+ AdaptiveAvgPool2d(1) if gap).
    ``pools``: per-layer pool flags (default: every layer pooled).  Only the last layer may go
    without its pool, and only in front of an NHWC tail (``nhwc_tail``: the LSTM towers' token
    rows) -- LSTMImageEncoder.cnn's last block (dino.py:75-115)."""

    def __init__(self, convs, hw, gap, conv_keys, bn_keys, pools=None, nhwc_tail=False):
        self.convs = convs            # [(cin, cout, k, pad)]
        self.hw = hw
        self.gap = gap
        self.conv_keys = conv_keys
        self.bn_keys = bn_keys
        self.pools = tuple(bool(p) for p in pools) if pools is not None else (True,) * len(convs)
        self.nhwc_tail = bool(nhwc_tail)
        if len(self.pools) != len(convs):
            raise ValueError(f"pools has {len(self.pools)} flags for {len(convs)} conv layers")
        if not all(self.pools[:-1]):
            raise ValueError("only the last conv layer may be unpooled")
        if not self.pools[-1] and (gap or not self.nhwc_tail):
            raise ValueError("an unpooled last layer needs nhwc_tail=True (and no gap)")

    def layer_dims(self):
        """[(H_in, Ho, Hpool)] per layer (square maps); Hpool = Ho for an unpooled layer."""
        out, h = [], self.hw
        for (_ci, _co, k, pad), pool in zip(self.convs, self.pools):
            ho = h + 2 * pad - k + 1
            hp = ho // 2 if pool else ho
            out.append((h, ho, hp))
            h = hp
        return out

    @property
    def flat(self):
        co = self.convs[-1][1]
        hp = self.layer_dims()[-1][2]
        return co if self.gap else co * hp * hp


CENTRAL_IMAGE_CONVS = [(1, 32, 5, 2), (32, 64, 5, 0)]
CENTRAL_AUDIO_CONVS = [(1, 8, 5, 2), (8, 16, 5, 2), (16, 32, 5, 2), (32, 64, 5, 2)]
CNN3_IMAGE_CONVS = [(1, 32, 3, 1), (32, 64, 3, 1), (64, 128, 3, 1)]
CNN3_AUDIO_CONVS = [(1, 32, 3, 1), (32, 64, 3, 1), (64, 128, 3, 1), (128, 256, 3, 1)]
PROJ_HIDDEN = 512


def central_stack(prefix, convs, hw):
    n = len(convs)
    return ConvStackSpec(convs, hw, False, [f"{prefix}.conv{i + 1}" for i in range(n)],
                         [f"{prefix}.bn{i + 1}" for i in range(n)])


def cnn3_stack(prefix, convs, hw):
    n = len(convs)
    return ConvStackSpec(convs, hw, True, [f"{prefix}.{4 * i}" for i in range(n)],
                         [f"{prefix}.{4 * i + 1}" for i in range(n)])


# ------------------------------------------------------------------ state-dict builders
def _dense(sd, key, out_f, in_f, k=None):
    sd[key + ".weight"] = ((out_f, in_f, k, k) if k else (out_f, in_f), "w")
    sd[key + ".bias"] = ((out_f,), "b")


def _bn(sd, key, c):
    sd[key + ".weight"] = ((c,), "bn_w")
    sd[key + ".bias"] = ((c,), "bn_b")
    sd[key + ".running_mean"] = ((c,), "rm")
    sd[key + ".running_var"] = ((c,), "rv")
    sd[key + ".num_batches_tracked"] = ((), "nbt")


def _central_lenet(sd, prefix, convs, fc1_in):
    for i, (ci, co, k, _p) in enumerate(convs, 1):
        _dense(sd, f"{prefix}.conv{i}", co, ci, k)
        _bn(sd, f"{prefix}.bn{i}", co)
    _dense(sd, f"{prefix}.fc1", 1024, fc1_in)   # built but never executed (with_head=False)
    _dense(sd, f"{prefix}.fc2", 10, 1024)


def _cnn3(sd, prefix, convs, out_dim):
    n = len(convs)
    for i, (ci, co, k, _p) in enumerate(convs):
        _dense(sd, f"{prefix}.{4 * i}", co, ci, k)
        _bn(sd, f"{prefix}.{4 * i + 1}", co)
    _dense(sd, f"{prefix}.{4 * n + 2}", out_dim, convs[-1][1])


def central_multimodal_sd(sd, prefix, E, D):
    _central_lenet(sd, f"{prefix}.image_encoder.0", CENTRAL_IMAGE_CONVS, 64 * 5 * 5)
    _dense(sd, f"{prefix}.image_encoder.1", E, 64 * 5 * 5)
    _central_lenet(sd, f"{prefix}.audio_encoder.0", CENTRAL_AUDIO_CONVS, 64 * 7 * 7)
    _dense(sd, f"{prefix}.audio_encoder.1", E, 64 * 7 * 7)
    _dense(sd, f"{prefix}.fusion.0", E, 2 * E)
    _dense(sd, f"{prefix}.fusion.3", D, E)


def simple_multimodal_sd(sd, prefix, E, D):
    """SimpleMultiModalEncoder (``--model multi_simple``): image_encoder(E), audio_encoder(E)
    (nn.Sequential 3x3 CNNs, Linear at index 14 / 18), fusion."""
    _cnn3(sd, f"{prefix}.image_encoder", CNN3_IMAGE_CONVS, E)
    _cnn3(sd, f"{prefix}.audio_encoder", CNN3_AUDIO_CONVS, E)
    _dense(sd, f"{prefix}.fusion.0", E, 2 * E)
    _dense(sd, f"{prefix}.fusion.3", D, E)


def gated_multimodal_sd(sd, prefix, E, D):
    """GatedMultiModalEncoder (``--model multi_simple_gated``, dino.py:237-259): the two scalar
    nn.Parameters are registered on the module itself, so they come before its submodules'
    keys in the reference's state_dict."""
    sd[f"{prefix}.gate_image"] = ((), "gate")
    sd[f"{prefix}.gate_audio"] = ((), "gate")
    simple_multimodal_sd(sd, prefix, E, D)


def cross_attention_multimodal_sd(sd, prefix, E, D):
    """CrossAttentionMultiModalEncoder (``--model multi_cross_attention``, dino.py:407-452):
    the two CrossModalAttention modules (q_proj Linear(E,E), kv_proj Linear(E,2E), 385-391)
    are created after fusion."""
    simple_multimodal_sd(sd, prefix, E, D)
    for att in XATTN_NAMES:
        _dense(sd, f"{prefix}.{att}.q_proj", E, E)
        _dense(sd, f"{prefix}.{att}.kv_proj", 2 * E, E)


# the two attention directions: (queries from, keys / values from) the cat halves
XATTN_NAMES = ("image_to_audio_attention", "audio_to_image_attention")
GATE_INIT = 0.5             # nn.Parameter(torch.tensor(0.5)), dino.py:242-243


# MODEL_MAP encoders that run on the engine (run_dino.py:530-540):
#   arch -> (image stack(prefix), image Linear key, audio stack(prefix), audio Linear key, sd builder)
MULTI_ENCODERS = {
    "multi_central": (lambda p: central_stack(f"{p}.image_encoder.0", CENTRAL_IMAGE_CONVS, 28), "image_encoder.1",
                      lambda p: central_stack(f"{p}.audio_encoder.0", CENTRAL_AUDIO_CONVS, 112), "audio_encoder.1",
                      central_multimodal_sd),
    "multi_simple": (lambda p: cnn3_stack(f"{p}.image_encoder", CNN3_IMAGE_CONVS, 28), "image_encoder.14",
                     lambda p: cnn3_stack(f"{p}.audio_encoder", CNN3_AUDIO_CONVS, 112), "audio_encoder.18",
                     simple_multimodal_sd),
    "multi_simple_gated": (lambda p: cnn3_stack(f"{p}.image_encoder", CNN3_IMAGE_CONVS, 28), "image_encoder.14",
                           lambda p: cnn3_stack(f"{p}.audio_encoder", CNN3_AUDIO_CONVS, 112), "audio_encoder.18",
                           gated_multimodal_sd),
    "multi_cross_attention": (lambda p: cnn3_stack(f"{p}.image_encoder", CNN3_IMAGE_CONVS, 28), "image_encoder.14",
                              lambda p: cnn3_stack(f"{p}.audio_encoder", CNN3_AUDIO_CONVS, 112),
                              "audio_encoder.18", cross_attention_multimodal_sd),
}
# the stage between the cat of the two towers' features and fusion ("mix"): absent = plain cat
MIX_KIND = {"multi_simple_gated": "gated", "multi_cross_attention": "xattn"}


def projection_head_sd(sd, prefix, in_dim, out_dim, hidden=PROJ_HIDDEN):
    _dense(sd, f"{prefix}.mlp.0", hidden, in_dim)
    _bn(sd, f"{prefix}.mlp.1", hidden)
    _dense(sd, f"{prefix}.mlp.4", out_dim, hidden)


HEAD_NAMES = {"mse": ("image_projection_head", "audio_projection_head"),
              "infonce": ("image_projection_head", "audio_projection_head"),
              "semi_supervised": ("image_classifier", "audio_classifier")}


def multimodal_dino_sd(mode, E, D, P, num_classes=10, encoder="multi_central"):
    build = MULTI_ENCODERS[encoder][4]
    sd = OrderedDict()
    sd["center"] = ((1, P), "center")
    build(sd, "student", E, D)
    build(sd, "teacher", E, D)
    projection_head_sd(sd, "student_projection", D, P)
    projection_head_sd(sd, "teacher_projection", D, P)
    if mode in HEAD_NAMES:
        hi, ha = HEAD_NAMES[mode]
        out = num_classes if mode == "semi_supervised" else P
        projection_head_sd(sd, hi, E, out)
        projection_head_sd(sd, ha, E, out)
    elif mode != "default":
        raise ValueError(f"unknown training mode {mode!r}")
    return sd


def image_encoder_sd(sd, prefix, out_dim):
    _cnn3(sd, f"{prefix}.encoder", CNN3_IMAGE_CONVS, 512)
    _dense(sd, f"{prefix}.projection.0", out_dim, 512)


def spectrogram_encoder_sd(sd, prefix, out_dim):
    _cnn3(sd, f"{prefix}.encoder", CNN3_AUDIO_CONVS, out_dim)


def unimodal_image_dino_sd(D, P):
    sd = OrderedDict()
    sd["center"] = ((1, P), "center")
    image_encoder_sd(sd, "student", D)
    image_encoder_sd(sd, "teacher", D)
    projection_head_sd(sd, "student_projection", D, P)
    projection_head_sd(sd, "teacher_projection", D, P)
    return sd


def spectrogram_central_sd(sd, prefix, out_dim):
    _central_lenet(sd, f"{prefix}.encoder.0", CENTRAL_AUDIO_CONVS, 64 * 7 * 7)
    _dense(sd, f"{prefix}.encoder.1", out_dim, 64 * 7 * 7)


# SpectrogramEncoderLSTM (dino.py:525-530 over LSTMAudioEncoder, 117-156): the first three blocks
# of the 3x3 audio CNN, Linear(128, LSTM_PROJ) + ReLU per pooled position, one bidirectional
# nn.LSTM(LSTM_PROJ, output_dim // 2) over the 14 x 14 positions, mean over them.
LSTM_PROJ = 64
LSTM_HIDDEN = tuple(range(16, 129, 16))          # hidden sizes the recurrence kernel serves
LSTM_DIMS = tuple(2 * h for h in LSTM_HIDDEN)    # = the supported output_dim values
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def lstm_hidden(out_dim):
    """Hidden size per direction for an output_dim, or ValueError naming the supported ones."""
    if out_dim not in LSTM_DIMS:
        raise ValueError(f"spectrogram_lstm: output_dim must be one of {LSTM_DIMS} (an even "
                         f"number whose half is a multiple of 16 up to 128), got {out_dim}")
    return out_dim // 2


def lstm_stack(prefix):
    convs = CNN3_AUDIO_CONVS[:3]
    n = len(convs)
    return ConvStackSpec(convs, 112, False, [f"{prefix}.{4 * i}" for i in range(n)],
                         [f"{prefix}.{4 * i + 1}" for i in range(n)])


def lstm_image_stack(prefix):
    """LSTMImageEncoder.cnn (dino.py:75-115): the 3x3 image CNN whose third block has no
    MaxPool2d -- 28 -> 14 -> 7 -> 7, i.e. 49 tokens of 128 channels.  Sequential indices: the
    missing pool shifts nothing before it, so the keys are cnn.0/1, 4/5, 8/9."""
    convs = CNN3_IMAGE_CONVS
    n = len(convs)
    return ConvStackSpec(convs, 28, False, [f"{prefix}.{4 * i}" for i in range(n)],
                         [f"{prefix}.{4 * i + 1}" for i in range(n)],
                         pools=(True, True, False), nhwc_tail=True)


def spectrogram_lstm_sd(sd, prefix, out_dim):
    H = lstm_hidden(out_dim)
    for i, (ci, co, k, _p) in enumerate(CNN3_AUDIO_CONVS[:3]):
        _dense(sd, f"{prefix}.encoder.cnn.{4 * i}", co, ci, k)
        _bn(sd, f"{prefix}.encoder.cnn.{4 * i + 1}", co)
    _dense(sd, f"{prefix}.encoder.feature_proj.0", LSTM_PROJ, 128)
    for suffix in ("", "_reverse"):
        for key, shape in zip(LSTM_KEYS, ((4 * H, LSTM_PROJ), (4 * H, H), (4 * H,), (4 * H,))):
            sd[f"{prefix}.encoder.lstm.{key}{suffix}"] = (shape, "lstm")


# UNIMODAL_MODEL_MAP encoders that run on the engine (run_dino.py:542-550):
#   kind -> (modality, stack builder(prefix), [Linear keys after the stack, relative to prefix],
#            state-dict builder)
# (spectrogram_lstm: the one Linear is feature_proj, per token; the LSTM follows it)
UNI_ENCODERS = {
    "image_simple": ("image", lambda p: cnn3_stack(f"{p}.encoder", CNN3_IMAGE_CONVS, 28),
                     ["encoder.14", "projection.0"], image_encoder_sd),
    "spectrogram_simple": ("audio", lambda p: cnn3_stack(f"{p}.encoder", CNN3_AUDIO_CONVS, 112),
                           ["encoder.18"], spectrogram_encoder_sd),
    "spectrogram_central": ("audio", lambda p: central_stack(f"{p}.encoder.0", CENTRAL_AUDIO_CONVS, 112),
                            ["encoder.1"], spectrogram_central_sd),
    "spectrogram_lstm": ("audio", lambda p: lstm_stack(f"{p}.encoder.cnn"),
                         ["encoder.feature_proj.0"], spectrogram_lstm_sd),
}
UNI_ALIASES = {"image": "image_simple", "audio": "spectrogram_simple"}

# SpectrogramEncoderViT (dino.py:532-546): Sequential(AudioViTEncoder(112, patch 8, embed 512,
# depth 4, heads 4) (dino_vit.py:122-177), Linear(512, output_dim)).  The tower's parameters:
# kinds "tok" (cls_token, pos_embed: zeros), "attn_w" (in_proj_weight: xavier-uniform), "attn_b"
# (in_proj_bias, out_proj.bias: zeros), "ln_w" / "ln_b" (LayerNorm: ones / zeros); the patch
# Conv2d and the Linears are "w" / "b".
VIT_AUDIO = dict(hw=112, patch=8, embed_dim=512, depth=4, heads=4)
VIT_MLP_RATIO = 4           # dim_feedforward = 4 * embed_dim (2048)
VIT_LN_EPS = 1e-5
VIT_DROPOUT = 0.1           # TransformerEncoder's default, on all four sites of a layer


def _ln(sd, key, c):
    sd[key + ".weight"] = ((c,), "ln_w")
    sd[key + ".bias"] = ((c,), "ln_b")


def vit_tower_sd(sd, prefix, hw, patch, embed_dim, depth, heads=None):
    """AudioViTEncoder / ViTEncoder state dict under ``prefix``: the two nn.Parameters of the
    module itself precede its submodules' keys."""
    E, T = embed_dim, (hw // patch) ** 2 + 1
    sd[f"{prefix}.cls_token"] = ((1, 1, E), "tok")
    sd[f"{prefix}.pos_embed"] = ((1, T, E), "tok")
    _dense(sd, f"{prefix}.patch_embed.projection", E, 1, patch)
    for i in range(depth):
        l = f"{prefix}.transformer.layers.{i}"
        sd[f"{l}.self_attn.in_proj_weight"] = ((3 * E, E), "attn_w")
        sd[f"{l}.self_attn.in_proj_bias"] = ((3 * E,), "attn_b")
        sd[f"{l}.self_attn.out_proj.weight"] = ((E, E), "w")
        sd[f"{l}.self_attn.out_proj.bias"] = ((E,), "attn_b")
        _dense(sd, f"{l}.linear1", VIT_MLP_RATIO * E, E)
        _dense(sd, f"{l}.linear2", E, VIT_MLP_RATIO * E)
        _ln(sd, f"{l}.norm1", E)
        _ln(sd, f"{l}.norm2", E)
    _ln(sd, f"{prefix}.transformer.norm", E)


def spectrogram_vit_sd(sd, prefix, out_dim):
    vit_tower_sd(sd, f"{prefix}.encoder.0", **VIT_AUDIO)
    _dense(sd, f"{prefix}.encoder.1", out_dim, VIT_AUDIO["embed_dim"])


# UNIMODAL_MODEL_MAP encoders on the ViT tower (avdino/vit.py), kept apart from UNI_ENCODERS,
# whose entries are all conv stacks:
#   kind -> (modality, tower prefix relative to the encoder's, tower dimensions,
#            [Linear keys after the tower], state-dict builder)
VIT_ENCODERS = {
    "spectrogram_vit": ("audio", "encoder.0", VIT_AUDIO, ["encoder.1"], spectrogram_vit_sd),
}


def uni_kinds():
    """Every unimodal encoder kind the engine runs (conv stacks and ViT towers)."""
    return tuple(UNI_ENCODERS) + tuple(VIT_ENCODERS)


def uni_modality(kind):
    kind = UNI_ALIASES.get(kind, kind)
    return (VIT_ENCODERS[kind] if kind in VIT_ENCODERS else UNI_ENCODERS[kind])[0]


def unimodal_dino_sd(kind, D, P):
    """UniModalDINO (models/dino.py:1257-1297) state dict over an UNI_ENCODERS or VIT_ENCODERS
    kind."""
    kind = UNI_ALIASES.get(kind, kind)
    build = VIT_ENCODERS[kind][4] if kind in VIT_ENCODERS else UNI_ENCODERS[kind][3]
    sd = OrderedDict()
    sd["center"] = ((1, P), "center")
    build(sd, "student", D)
    build(sd, "teacher", D)
    projection_head_sd(sd, "student_projection", D, P)
    projection_head_sd(sd, "teacher_projection", D, P)
    return sd


def simclr_sd(D, P):
    sd = OrderedDict()
    image_encoder_sd(sd, "image_encoder", D)
    spectrogram_encoder_sd(sd, "audio_encoder", D)
    projection_head_sd(sd, "image_projection_head", D, P)
    projection_head_sd(sd, "audio_projection_head", D, P)
    return sd
