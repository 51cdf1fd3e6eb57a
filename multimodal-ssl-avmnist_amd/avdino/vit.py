"""The ViT tower (AudioViTEncoder / ViTEncoder, reference models/dino_vit.py:27-177) with explicit
forward and backward over libavdino (csrc/vit.hip + the dense GEMMs): patch rows, one GEMM, the
cls / position tokens, ``depth`` post-norm nn.TransformerEncoderLayer(gelu, batch_first) layers,
the final LayerNorm of the cls rows.

The tower knows nothing of an engine: it takes a workspace, a parameter store, a key prefix and
its dimensions, so the unimodal encoder (embed_dim 512) and a later multimodal one
(embed_dim = encoder_output_dim) instantiate the same class.

``attention`` picks the attention kernels (ATTENTION_KINDS): "exact" = avd_mhsa_* (csrc/vit.hip, f32
sums on the VALU in both modes, the default) or "mfma" = avd_mhsa_mfma_* (csrc/mhsa_mfma.hip, bf16
tensor-core kernels; bf16 activations only).  Same operands, lse, seeds and masks either way.

Dropout sites and seeds.  A layer has four: "attn" on the attention probabilities, "sa" on the
attention block's output (dropout1), "ff1" inside the MLP (dropout), "ff2" on the MLP's output
(dropout2).  ``seeds`` = (p, base, seed_off, role): site s (0 attn, 1 sa, 2 ff1, 3 ff2) of layer
i draws from the 64-bit seed
    site_seed(base, role, i, s) = (base mod 2^48) + ((1 + 64 role + 4 i + s) << 48)
plus the device counter *seed_off (StepState.seed_off advances by 16 per step, far below 2^48, so
a replayed graph draws fresh masks and no two sites ever share a seed; the engine's other dropouts
use base + small constants, i.e. site number 0).  role 0 is the student, 1 the teacher -- the
reference's teacher is a train-mode module, so its dropout is active too, with masks of its own.
``seeds=None`` (eval passes) draws nothing.

Activation footprint (f32 elements per token row, R = N * T rows, E = embed_dim, F = 4E):
  saved per layer for the backward: qkv 3E + ctx E + h1 E + z1 E + f1 F + f2 F + h2 E + z2 E
                                     = 8E + 2F = 16E      (+ lse, mean, rstd: heads + 4 per row)
  shared forward scratch:           a E + m E, tokens E, patch rows and embeddings (P*P + E)
  backward scratch:                 dh, dh1, dm, dt 4E + dqkv 3E + df F = 11E
  a pass without the backward (teacher, eval) reuses one layer's buffers: 16E + 3E per row.
activation_elems() returns these sums; DESIGN 3.11 has the numbers at the config's batch size.
"""
import torch

from . import ops

F32 = torch.float32
SITES = ("attn", "sa", "ff1", "ff2")
MAX_DEPTH = 16              # layers a role's 64 site numbers cover
ATTENTION_KINDS = ("exact", "mfma")     # avd_mhsa_* (f32 VALU sums) | avd_mhsa_mfma_* (bf16 MFMA)


def site_seed(base, role, layer, site):
    return (int(base) & 0xFFFFFFFFFFFF) + ((1 + 64 * role + 4 * layer + SITES.index(site)) << 48)


def tokens(hw, patch):
    return (hw // patch) ** 2 + 1


class ViTTower:
    def __init__(self, prefix, hw, patch, embed_dim, depth, heads, act_dtype, gemm_mode, mlp_ratio=4,
                 eps=1e-5, attention="exact"):
        if attention not in ATTENTION_KINDS:
            raise ValueError(f"ViT: attention must be one of {ATTENTION_KINDS} (got {attention!r})")
        if attention == "mfma" and act_dtype != torch.bfloat16:
            raise ValueError("ViT: attention='mfma' is a bf16 kernel; it has no f32 mode "
                             f"(activation dtype {act_dtype})")
        self.attention = attention
        if hw % patch != 0:
            raise ValueError(f"ViT: the map size {hw} is no multiple of the patch size {patch}")
        if embed_dim % heads != 0 or embed_dim // heads not in ops.MHSA_HEAD_DIMS:
            raise ValueError(f"ViT: embed_dim / heads must be one of {ops.MHSA_HEAD_DIMS} "
                             f"(got {embed_dim} / {heads})")
        if embed_dim % 32 != 0 or embed_dim > ops.LN_EMAX:
            raise ValueError(f"ViT: embed_dim must be a multiple of 32 up to {ops.LN_EMAX} (got {embed_dim})")
        self.prefix, self.hw, self.patch = prefix, hw, patch
        if not 1 <= depth <= MAX_DEPTH:
            raise ValueError(f"ViT: depth must be 1..{MAX_DEPTH} (got {depth})")
        self.E, self.depth, self.heads = embed_dim, depth, heads
        self.dh = embed_dim // heads
        self.F = mlp_ratio * embed_dim
        self.T = tokens(hw, patch)
        if self.T > ops.MHSA_TMAX:
            raise ValueError(f"ViT: {self.T} tokens; the attention kernels serve up to {ops.MHSA_TMAX}")
        self.act, self.gm = act_dtype, gemm_mode
        self.bf16 = act_dtype == torch.bfloat16
        self.eps = eps
        self.scale = float(self.dh) ** -0.5

    # ---- sizes
    def activation_elems(self, N, train):
        """f32 elements the tower keeps in the workspace for N sequences (module docstring)."""
        E, F, T, R = self.E, self.F, self.T, N * self.T
        layer = R * (8 * E + 2 * F) + N * self.heads * T + 4 * R
        shared = R * 3 * E + N * (T - 1) * (self.patch ** 2 + E) + 3 * N * E
        if not train:
            return layer + shared
        return self.depth * layer + shared + R * (7 * E + F) + N * (T - 1) * E

    def _key(self, i, name):
        return f"{self.prefix}.transformer.layers.{i}.{name}"

    @staticmethod
    def _seed(seeds, i, site):
        if seeds is None:
            return 0.0, 0, None
        p, base, off, role = seeds
        return float(p), site_seed(base, role, i, site), off

    # ---- the chosen attention family
    def _mhsa_fwd(self, q, k, v, ctx, lse, N, p, seed, off):
        if self.attention == "mfma":
            return ops.mhsa_mfma_fwd(q, k, v, ctx, lse, N, self.heads, self.T, self.dh, self.scale, p, seed, off)
        return ops.mhsa_fwd(q, k, v, ctx, lse, N, self.heads, self.T, self.dh, self.scale, self.bf16, p, seed,
                            off)

    def _mhsa_bwd_ws(self, N):
        ws = ops.mhsa_mfma_bwd_ws if self.attention == "mfma" else ops.mhsa_bwd_ws
        return ws(N, self.heads, self.T, self.dh)

    def _mhsa_bwd(self, dout, q, k, v, lse, dq, dk, dv, ws, N, p, seed, off):
        if self.attention == "mfma":
            return ops.mhsa_mfma_bwd(dout, q, k, v, lse, dq, dk, dv, ws, N, self.heads, self.T, self.dh,
                                     self.scale, p, seed, off)
        return ops.mhsa_bwd(dout, q, k, v, lse, dq, dk, dv, ws, N, self.heads, self.T, self.dh, self.scale,
                            self.bf16, p, seed, off)

    # ---- forward
    def forward(self, ws, store, tag, x, N, train, seeds=None):
        """x: the staged one-channel maps [N, hw, hw] (act dtype).  Returns (cls [N, E] f32: the
        final LayerNorm's cls rows, ctx for backward or None when not train)."""
        E, F, T, P, heads, dh = self.E, self.F, self.T, self.patch, self.heads, self.dh
        R, Tp, pre, st = N * T, T - 1, self.prefix, store
        patches = ws.get(f"{tag}.patch", N * Tp * P * P)
        ops.vit_patchify(x, patches, N, self.hw, self.hw, P)
        pe = ws.get(f"{tag}.pe", N * Tp * E)
        wp = st[f"{pre}.patch_embed.projection.weight"].view(E, P * P)
        ops.linear_fwd(patches, wp, st[f"{pre}.patch_embed.projection.bias"], pe, N * Tp, mode=self.gm)
        h = ws.get(f"{tag}.tok", R * E)
        ops.vit_tokens_fwd(pe, st[f"{pre}.cls_token"], st[f"{pre}.pos_embed"], h, N, T, E)
        a = ws.get(f"{tag}.a", R * E)
        m = ws.get(f"{tag}.m", R * E)
        layers = []
        for i in range(self.depth):
            def buf(name, n, i=i):
                return ws.get(f"{tag}.l{i}.{name}" if train else f"{tag}.l.{name}", n)
            c = dict(x=h)
            qkv = c["qkv"] = buf("qkv", R * 3 * E)
            ops.linear_fwd(h, st[self._key(i, "self_attn.in_proj_weight")],
                           st[self._key(i, "self_attn.in_proj_bias")], qkv, R, mode=self.gm)
            att = c["ctx"] = buf("ctx", R * E)
            lse = c["lse"] = buf("lse", N * heads * T) if train else None
            p, seed, off = self._seed(seeds, i, "attn")
            self._mhsa_fwd((qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E), (att, 0, E), lse, N, p, seed,
                           off)
            ops.linear_fwd(att, st[self._key(i, "self_attn.out_proj.weight")],
                           st[self._key(i, "self_attn.out_proj.bias")], a, R, mode=self.gm)
            h1 = c["h1"] = buf("h1", R * E)
            for n in ("z1", "z2"):
                c[n] = buf(n, R * E) if train else None
            for n in ("mean1", "rstd1", "mean2", "rstd2"):
                c[n] = buf(n, R) if train else None
            p, seed, off = self._seed(seeds, i, "sa")
            ops.ln_fwd(h, a, st[self._key(i, "norm1.weight")], st[self._key(i, "norm1.bias")], h1, R, E,
                       c["z1"], c["mean1"], c["rstd1"], self.eps, p, seed, off)
            f1 = c["f1"] = buf("f1", R * F)
            ops.linear_fwd(h1, st[self._key(i, "linear1.weight")], st[self._key(i, "linear1.bias")], f1, R,
                           mode=self.gm)
            f2 = c["f2"] = buf("f2", R * F)
            p, seed, off = self._seed(seeds, i, "ff1")
            ops.gelu_fwd(f1, f2, R, F, p, seed, off)
            ops.linear_fwd(f2, st[self._key(i, "linear2.weight")], st[self._key(i, "linear2.bias")], m, R,
                           mode=self.gm)
            h2 = buf("h2", R * E)
            p, seed, off = self._seed(seeds, i, "ff2")
            ops.ln_fwd(h1, m, st[self._key(i, "norm2.weight")], st[self._key(i, "norm2.bias")], h2, R, E,
                       c["z2"], c["mean2"], c["rstd2"], self.eps, p, seed, off)
            layers.append(c)
            h = h2
        out = ws.get(f"{tag}.cls", N * E)
        zf = ws.get(f"{tag}.zf", N * E) if train else None
        mf = ws.get(f"{tag}.meanf", N) if train else None
        rf = ws.get(f"{tag}.rstdf", N) if train else None
        ops.ln_fwd(h, None, st[f"{pre}.transformer.norm.weight"], st[f"{pre}.transformer.norm.bias"], out,
                   N, E, zf, mf, rf, self.eps, x_ld=T * E)
        if not train:
            return out.view(N, E), None
        return out.view(N, E), dict(N=N, layers=layers, patches=patches, zf=zf, meanf=mf, rstdf=rf,
                                    seeds=seeds)

    def forward_eval(self, ws, store, tag, x, N):
        return self.forward(ws, store, tag, x, N, False, None)[0]

    # ---- backward
    def backward(self, ws, store, ctx, dcls):
        """dcls [N, E]: the gradient of forward()'s output.  Writes every parameter gradient of the
        tower into the store's gradient arena (the input is data: no input gradient)."""
        E, F, T, P, heads, dh = self.E, self.F, self.T, self.patch, self.heads, self.dh
        N, seeds, pre, st = ctx["N"], ctx["seeds"], self.prefix, store
        R, Tp = N * T, T - 1
        g = st.grad_of
        lnws = ws.get("vit.lnws", ops.ln_bwd_ws(R, E))
        dhb = ws.get("vit.dh", R * E)
        dh1 = ws.get("vit.dh1", R * E)
        dm = ws.get("vit.dm", R * E)
        dt = ws.get("vit.dt", R * E)
        dqkv = ws.get("vit.dqkv", R * 3 * E)
        df = ws.get("vit.df", R * F)
        aws = ws.get("vit.aws", self._mhsa_bwd_ws(N))
        # the final LayerNorm saw the cls rows only: every other token row's gradient is zero
        dhb.zero_()
        ops.ln_bwd(dcls.reshape(-1), ctx["zf"], ctx["meanf"], ctx["rstdf"], st[f"{pre}.transformer.norm.weight"],
                   dhb, None, g(f"{pre}.transformer.norm.weight"), g(f"{pre}.transformer.norm.bias"), lnws,
                   N, E, dx_ld=T * E)
        for i in reversed(range(self.depth)):
            c = ctx["layers"][i]
            k = lambda name, i=i: self._key(i, name)        # noqa: E731
            # h2 = LN2(h1 + drop(m)),  m = f2 W2^T + b2,  f2 = drop(gelu(f1)),  f1 = h1 W1^T + b1
            p, seed, off = self._seed(seeds, i, "ff2")
            ops.ln_bwd(dhb, c["z2"], c["mean2"], c["rstd2"], st[k("norm2.weight")], dh1, dm,
                       g(k("norm2.weight")), g(k("norm2.bias")), lnws, R, E, p, seed, off)
            ops.linear_bwd(dm, c["f2"], st[k("linear2.weight")], g(k("linear2.weight")),
                           g(k("linear2.bias")), df, R, mode=self.gm)
            p, seed, off = self._seed(seeds, i, "ff1")
            ops.gelu_bwd(c["f1"], df, df, R, F, p, seed, off)          # elementwise, in place
            ops.linear_bwd(df, c["h1"], st[k("linear1.weight")], g(k("linear1.weight")),
                           g(k("linear1.bias")), dt, R, mode=self.gm)
            ops.axpy(dh1, dt)
            # h1 = LN1(x + drop(a)),  a = ctx Wo^T + bo,  ctx = attention(qkv),  qkv = x Win^T + bin
            p, seed, off = self._seed(seeds, i, "sa")
            ops.ln_bwd(dh1, c["z1"], c["mean1"], c["rstd1"], st[k("norm1.weight")], dhb, dm,
                       g(k("norm1.weight")), g(k("norm1.bias")), lnws, R, E, p, seed, off)
            ops.linear_bwd(dm, c["ctx"], st[k("self_attn.out_proj.weight")],
                           g(k("self_attn.out_proj.weight")), g(k("self_attn.out_proj.bias")), dt, R,
                           mode=self.gm)
            p, seed, off = self._seed(seeds, i, "attn")
            qkv = c["qkv"]
            self._mhsa_bwd((dt, 0, E), (qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E), c["lse"],
                           (dqkv, 0, 3 * E), (dqkv, E, 3 * E), (dqkv, 2 * E, 3 * E), aws, N, p, seed, off)
            ops.linear_bwd(dqkv, c["x"], st[k("self_attn.in_proj_weight")],
                           g(k("self_attn.in_proj_weight")), g(k("self_attn.in_proj_bias")), dh1, R,
                           mode=self.gm)
            ops.axpy(dhb, dh1)
        # tokens: dpos = sum over the sequences, dcls_token = its row 0, patch rows compacted
        gpos = g(f"{pre}.pos_embed").view(-1)
        ops.sum_rows(dhb, N, T * E, gpos)
        g(f"{pre}.cls_token").view(-1).copy_(gpos[:E])
        dpe = ws.get("vit.dpe", N * Tp * E)
        ops.vit_tokens_bwd(dhb, dpe, N, T, E)
        ops.linear_bwd(dpe, ctx["patches"], st[f"{pre}.patch_embed.projection.weight"].view(E, P * P),
                       g(f"{pre}.patch_embed.projection.weight").view(E, P * P),
                       g(f"{pre}.patch_embed.projection.bias"), None, N * Tp, mode=self.gm)
