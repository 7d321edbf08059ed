"""Spectre-ViT -- mirror of reference spectre_vit/models/spectre/spectre.py.

Class names, constructor arguments, forward signatures and state_dict keys follow the reference
(SURVEY.md 8b); the arithmetic runs in libspv_hip.so.  One labelled extension: ``mixer=`` on
SpectreViT / SpectreEncoderLayer selects the token mixer ("permut" = the reference's HEAD default
MHPermutMix, "fft" = FNet Re(fft2), "dwt_embed" / "dwt_token" = Haar DWT, "attention" = self-attention over
the tokens with nn.MultiheadAttention's parameters, "hadamard" = the 2-D Walsh-Hadamard transform of the reference's hadamar.py,
"filter" = a learnable frequency-domain filter along the tokens, GFNet's global filter) -- the modes the reference's docstring lists
(spectre.py:29-35; its undefined "fft_mh" aside) and BASELINE.json benchmarks.
"""
import torch
import torch.nn as nn
from torch.nn.modules.transformer import _get_activation_fn, _get_clones

from spectre_vit import hip_ops, shadows
from spectre_vit.models.spectre.layers import MHPermutMix, SpectreLinear
from spectre_vit.modules.mixers import FNetMixer, GlobalFilterMixer, HaarDWTMixer, HadamardMixer, SelfAttentionMixer

MIXERS = ("permut", "fft", "dwt_embed", "dwt_token", "attention", "hadamard", "filter")


class Transpose(nn.Module):
    """reference spectre.py:8-14 (pure view op)."""

    def __init__(self, dims=(-2, -1)):
        super(Transpose, self).__init__()
        self.dims = dims

    def forward(self, x):
        return x.transpose(self.dims[0], self.dims[1])


def _make_mixer(mixer, d_model, seq_length, nhead, dwt_levels, dwt_mode="passthrough", dropout=0.0):
    if mixer == "permut":
        return MHPermutMix(d_model, seq_length, nhead, d_model)
    if mixer == "fft":
        return FNetMixer()
    if mixer == "dwt_embed":
        return HaarDWTMixer("embed", dwt_levels, dwt_mode)
    if mixer == "dwt_token":
        return HaarDWTMixer("token", dwt_levels, dwt_mode)
    if mixer == "attention":
        return SelfAttentionMixer(d_model, nhead, dropout)
    if mixer == "hadamard":
        return HadamardMixer()
    if mixer == "filter":
        return GlobalFilterMixer(seq_length, d_model)
    raise ValueError(f"mixer must be one of {MIXERS}, got {mixer!r}")


class SpectreEncoderLayer(nn.Module):
    """x = norm1(mix(x)) + x ; x = norm2(x + linear3(linear1(x)))   (reference spectre.py:29-73)."""

    def __init__(self, seq_length, d_model, nhead, dim_feedforward, dropout, activation, mixer="permut", dwt_levels=1,
                 dwt_mode="passthrough"):
        super().__init__()
        bias = True
        layer_norm_eps = 1e-5
        self.mixer = mixer
        self.mix_layer = _make_mixer(mixer, d_model, seq_length, nhead, dwt_levels, dwt_mode, dropout)
        self.linear1 = SpectreLinear(d_model, dim_feedforward)
        self.linear3 = SpectreLinear(dim_feedforward, d_model)

        self.norm1 = nn.LayerNorm(d_model, eps=layer_norm_eps, bias=bias)
        self.norm2 = nn.LayerNorm(d_model, eps=layer_norm_eps, bias=bias)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        # dropout1/dropout2 are fused into the SpectreLinear tail kernel (same mask semantics, own RNG stream)
        self.linear1.drop_p = dropout
        self.linear3.drop_p = dropout

        if isinstance(activation, str):
            activation = _get_activation_fn(activation)
        self.activation = activation  # resolved but never called, as in the reference (spectre.py:60-63)

    def forward(self, x):
        return self._ff(self._mix(x))

    def forward_cls(self, x):
        """row 0 of forward(x), as (B, E): the mixer half over all tokens, the feed-forward half -- which works row by row -- at the CLS
        rows only.  For the LAST layer of a stack whose consumer reads nothing but the CLS row (SpectreViT, reference spectre.py:198)."""
        if self.mixer == "permut" and self.mix_layer.concat_dim <= self.mix_layer.embed_dim * self.mix_layer.token_dim:
            # MHPermutMix is a gather + a row-wise SpectreLinear: its own row 0 needs one gathered row, not 65
            m0, x0 = self.mix_layer.forward_cls(hip_ops.cast(x, hip_ops.compute_dtype(x)))
            return self._ff(hip_ops.add_layernorm(m0, x0, self.norm1.weight, self.norm1.bias, 0))
        if self.mixer == "fft":
            xc = hip_ops.cast(x, hip_ops.compute_dtype(x))
            if hip_ops.fnet_cls_ok(xc):
                # row 0 of Re(fft2(x)) is one FFT of the token sum: the mixer half as one pass over x, its backward one write
                return self._ff(hip_ops.FNetClsFn.apply(xc, self.norm1.weight, self.norm1.bias))
        if self.mixer == "hadamard":
            xc = hip_ops.cast(x, hip_ops.compute_dtype(x))
            if hip_ops.hadamard_cls_ok(xc):
                # row 0 of H is all ones: one transform of the token sum, as for the FFT mixer
                return self._ff(hip_ops.HadamardClsFn.apply(xc, self.norm1.weight, self.norm1.bias, self.mix_layer.normalize))
        if self.mixer == "attention":
            xc = hip_ops.cast(x, hip_ops.compute_dtype(x))
            if hip_ops.attn_row0_ok(xc, self.mix_layer.num_heads):
                # K and V over every row, the query, the attention and everything after it at the CLS rows only
                m0, x0 = self.mix_layer.forward_cls(xc)
                return self._ff(hip_ops.add_layernorm(m0, x0, self.norm1.weight, self.norm1.bias, 0))
        if self.mixer == "dwt_embed":
            # the Haar transform along the embedding axis is row-wise too: the whole layer runs at the CLS rows
            x0 = hip_ops.TakeClsFn.apply(hip_ops.cast(x, hip_ops.compute_dtype(x)))
            return self._ff(self._mix(x0.unsqueeze(1)).squeeze(1))
        return self._ff(hip_ops.TakeClsFn.apply(self._mix(x)))

    def _mix(self, x):
        x = hip_ops.cast(x, hip_ops.compute_dtype(x))
        if self.mixer == "fft":  # mixer + norm1 + residual as one autograd node (residual gradient folded into the FFT kernel)
            x = hip_ops.FNetResidualFn.apply(x, self.norm1.weight, self.norm1.bias)
        elif self.mixer == "hadamard" and hip_ops.hadamard_ln_ok(x):   # the same node for the Walsh-Hadamard mixer, inside its window
            x = hip_ops.HadamardResidualFn.apply(x, self.norm1.weight, self.norm1.bias, self.mix_layer.normalize)
        elif self.mixer == "dwt_embed" and hip_ops.haar_ln_ok(x, self.mix_layer.axis, self.mix_layer.levels):
            x = hip_ops.HaarResidualFn.apply(x, self.norm1.weight, self.norm1.bias)   # mixer + norm1 + residual as one row kernel each way
        else:
            x = hip_ops.add_layernorm(self.mix_layer(x), x, self.norm1.weight, self.norm1.bias, 0)
        return x

    def _ff(self, x):
        l1, l3 = self.linear1.local_head, self.linear3.local_head
        mult = 8 if x.dtype == torch.bfloat16 else 4
        if (l1[0].in_features % mult == 0 and l1[0].out_features % mult == 0):
            # linear1 -> linear3 -> + x -> norm2 as one autograd node (spectre.py:67,70-73)
            p = self.linear1.drop_p if self.training else 0.0
            return hip_ops.FFResidualFn.apply(x, l1[0].weight, l1[0].bias, l1[1].weight, l1[1].bias, l3[0].weight, l3[0].bias,
                                              l3[1].weight, l3[1].bias, self.norm2.weight, self.norm2.bias, p)
        return hip_ops.add_layernorm(self._ff_block(x), x, self.norm2.weight, self.norm2.bias, 1)

    def _ff_block(self, x: torch.Tensor) -> torch.Tensor:
        return self.linear3(self.linear1(x))


class SpectreEncoder(nn.Module):
    """Stack of cloned layers + global residual ``output + src`` (reference spectre.py:76-103)."""

    __constants__ = ["norm"]

    def __init__(self, encoder_layer, num_layers: int, norm=None) -> None:
        super().__init__()
        self.layers = _get_clones(encoder_layer, num_layers)
        self.num_layers = num_layers
        self.norm = norm

    def forward(self, src: torch.Tensor):
        src = hip_ops.cast(src, hip_ops.compute_dtype(src))
        output = src
        for mod in self.layers:
            output = mod(output)
        if self.norm is not None:
            output = self.norm(output)
        return hip_ops.AddFn.apply(output, src)

    def forward_cls(self, src: torch.Tensor):
        """(forward(src))[:, 0, :] without forming the other rows of the global residual (SpectreViT reads nothing else,
        reference spectre.py:198): same numbers, one (B, N, E) add and one gradient accumulation fewer per step."""
        src = hip_ops.cast(src, hip_ops.compute_dtype(src))
        output, src_cls = hip_ops.TapClsFn.apply(src)
        output = self._stack_cls(output)
        return hip_ops.ClsAddFn.apply(output, src_cls)

    def _stack_cls(self, output):
        """the layer stack for a consumer of the CLS row: (B, 1, E) when the last layer's feed-forward half ran at the CLS rows only
        (hip_ops.LAST_LAYER_CLS_ONLY), the full (B, N, E) otherwise"""
        layers = list(self.layers)
        cls_only = hip_ops.LAST_LAYER_CLS_ONLY and len(layers) > 0 and output.is_cuda
        for mod in (layers[:-1] if cls_only else layers):
            output = mod(output)
        if cls_only:
            output = layers[-1].forward_cls(output).unsqueeze(1)
        if self.norm is not None:
            output = self.norm(output)
        return output

    def forward_cls_parts(self, src: torch.Tensor):
        """forward_cls without the final CLS-row add: (stack output (B, N, E) or (B, 1, E), CLS row of the stack input (B, E)) for a consumer
        that folds the add into its own kernel (the class head, hip_ops.ClsHeadFn)."""
        src = hip_ops.cast(src, hip_ops.compute_dtype(src))
        output, src_cls = hip_ops.TapClsFn.apply(src)
        return self._stack_cls(output), src_cls


class SpectralPatchEmbed(nn.Module):
    """Per-patch Re(rfft2 ortho) * learnable frequency weights -> Linear -> CLS + position (+dropout)
    (reference spectre.py:106-156).  The fixed DFT map and the frequency weights are folded into the
    projection matrix (spv_spectral_fold), so the whole embedding is one patch GEMM."""

    def __init__(self, embed_dim, patch_size, num_patches, dropout, in_channels):
        super().__init__()
        self.P = patch_size
        self.embed_dim = embed_dim
        self.in_channels = in_channels
        self.freq_weight_h = nn.Parameter(torch.ones(self.P))
        self.freq_weight_w = nn.Parameter(torch.ones(self.P // 2 + 1))
        self.proj = nn.Linear(in_channels * self.P * (self.P // 2 + 1), embed_dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, embed_dim))
        self.position_embeddings = nn.Parameter(torch.randn(1, num_patches + 1, embed_dim))
        self.dropout = nn.Dropout(dropout)
        # extension: uint8 NHWC batches straight from the loader are normalised inside the patch gather
        self.pixel_norm = hip_ops.PixelNorm()

    def forward(self, x):
        C = x.shape[-1] if x.dtype == torch.uint8 else x.shape[1]
        w_full = hip_ops.SpectralFoldFn.apply(self.proj.weight, self.freq_weight_h, self.freq_weight_w, C, self.P)
        return hip_ops.patch_embed(x, w_full, self.proj.bias, self.cls_token, self.position_embeddings, self.P, self.pixel_norm,
                                   self.dropout.p if self.training else 0.0)   # the nn.Dropout of spectre.py:156, inside the same node

    def _prologue_sources(self, x):
        """what forward(x) hands SpectralFoldFn and patch_embed, for hip_ops.step_prologue (which launches their small kernels ahead
        of the forward): (proj_w, fh, fw, chans, patch) and (bias, cls, pos).  None: a batch the prologue does not serve (uint8)."""
        if x.dtype == torch.uint8 or x.dim() != 4:
            return None
        return ((self.proj.weight, self.freq_weight_h, self.freq_weight_w, x.shape[1], self.P),
                (self.proj.bias, self.cls_token, self.position_embeddings))


class SpectreViT(nn.Module):
    """reference spectre.py:159-202."""

    def __init__(self, img_size=32, patch_size=4, in_channels=3, num_classes=10, embed_dim=768, num_encoders=12,
                 num_heads=12, hidden_dim=3072, dropout=0.1, activation="gelu", mixer="permut", dwt_levels=1, dwt_mode="passthrough"):
        super().__init__()
        num_patches = (img_size // patch_size) ** 2
        self.embeddings_block = SpectralPatchEmbed(embed_dim, patch_size, num_patches, dropout, in_channels)
        encoder_layer = SpectreEncoderLayer(seq_length=num_patches + 1, d_model=embed_dim, nhead=num_heads,
                                            dim_feedforward=hidden_dim, dropout=dropout, activation=activation,
                                            mixer=mixer, dwt_levels=dwt_levels, dwt_mode=dwt_mode)
        self.encoder_blocks = SpectreEncoder(encoder_layer, num_layers=num_encoders)
        self.mlp_head = nn.Sequential(SpectreLinear(embed_dim, num_classes))
        self.mlp_head[0].out_fp32 = True  # logits leave in fp32, as they do under stock autocast (LayerNorm output)

    def _shadow_weights(self):
        """the encoder's nn.Linear weights whose bf16 (W, W^T) copies the GEMMs read (rebuilt every training forward)"""
        cand = self.__dict__.get("_shadow_candidates")
        if cand is None or cand[0] != len(self.encoder_blocks.layers):
            # the module walk costs the host 0.1 ms per step (the eager, data-parallel path is host-bound): done once per stack
            mods = [mod for layer in self.encoder_blocks.layers for mod in layer.modules() if isinstance(mod, (SpectreLinear, SelfAttentionMixer))]
            cand = self.__dict__["_shadow_candidates"] = (len(self.encoder_blocks.layers), mods)
        ws = []
        for mod in cand[1]:
            # (looked up every time: a caller may have replaced the parameter)
            for w in ((mod.in_proj_weight, mod.out_proj.weight) if isinstance(mod, SelfAttentionMixer) else (mod.local_head[0].weight,)):
                if w.requires_grad and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0:
                    ws.append(w)
        return ws

    def _observed(self):
        """True when somebody watches the modules the fast paths below step around: a forward (pre-)hook on the layer stack, one of its
        layers, the class head -- or a global module hook.  SpectreViT then runs the reference's own call sequence
        (``encoder_blocks(x)`` -> ``x[:, 0, :]`` -> ``mlp_head(cls)``, spectre.py:196-199) through every module's ``__call__`` with every
        row of the last layer computed, so a hook sees the tensors the reference would hand it.  Same logits and gradients."""
        from torch.nn.modules import module as _m
        if _m._global_forward_hooks or _m._global_forward_pre_hooks:
            return True
        watched = [self.encoder_blocks, *self.encoder_blocks.layers, self.mlp_head, *self.mlp_head]
        if self.encoder_blocks.layers:
            watched += list(self.encoder_blocks.layers[-1].children())
        return any(w._forward_hooks or w._forward_pre_hooks for w in watched)

    def forward(self, x, return_features=False):
        if torch.is_grad_enabled() and x.is_cuda and torch.is_autocast_enabled("cuda"):
            shadows.refresh_weight_shadows(self, self._shadow_weights)  # all layers' bf16 weight copies in one launch
        x = self.embeddings_block(x)
        if self._observed():
            x = self.encoder_blocks(x)
            cls_token = x[:, 0, :]
            x = self.mlp_head(cls_token)
            return (x, cls_token) if return_features else x
        head = self.mlp_head[0] if len(self.mlp_head) == 1 and isinstance(self.mlp_head[0], SpectreLinear) else None
        if (head is not None and (head.drop_p == 0.0 or not self.training) and x.is_cuda
                and hip_ops.small_head_ok(x.shape[0], head.out_channels, head.in_channels)):
            # the class head over the B CLS rows: CLS add + Linear + LayerNorm + GELU + pooled skip in one launch (fp32 logits)
            output, src_cls = self.encoder_blocks.forward_cls_parts(x)
            lin, ln = head.local_head[0], head.local_head[1]
            x, cls_token = hip_ops.ClsHeadFn.apply(output, src_cls, lin.weight, lin.bias, ln.weight, ln.bias)
        else:
            cls_token = self.encoder_blocks.forward_cls(x)
            x = self.mlp_head(cls_token)
        if return_features:
            return x, cls_token
        return x
