"""SpectreBranch -- mirror of reference spectre_vit/models/spectre_branch/spectre_branch.py:1-224.

Same classes, constructor arguments, attribute names and registration order (state_dict keys, shapes and the same-seed
initialisation match the reference's).  The forward passes run on libspv_hip.so through spectre_vit.hip_ops: the image spectrum,
the 3x3 convolution chain and the token pooling on the kernels of csrc/spv_branch.hip, the encoder's Linear / LayerNorm / dropout
on the library's existing GEMM and row kernels.

Reference behaviour kept: the encoder layer has no activation (:79-89 never calls it), ``mix_layer`` and ``dropout1`` are never
used (``mix_layer`` receives no gradient, so AdamW leaves it untouched), and ``SpectreMix`` is defined but unused.  The
reference's own limits are reported by the constructors: ``embed_dim`` must be 768 (:105), ``in_channels`` 3 (:102), and the
conv chain must not empty (each stage shrinks the spectrum by 2 in both directions).
"""
import torch
import torch.nn as nn
from torch.nn.modules.transformer import _get_activation_fn, _get_clones

from spectre_vit import branch_ops, hip_ops
from spectre_vit.models.spectre.spectre import Transpose
from spectre_vit.modules.patch_embeddings import PatchEmbedding


class SpectreMix(nn.Module):
    """x + proj_head(cat([head(x) for head in head_linears], -1))   (reference :9-32; unused by the model)"""

    def __init__(self, in_channels, num_heads, seq_length):
        super().__init__()
        self.num_heads = num_heads
        self.in_channels = in_channels
        shrink = 4
        self.head_linears = nn.ModuleList([nn.Linear(in_channels, in_channels // shrink) for _ in range(self.num_heads)])
        self.proj_head = nn.Linear(self.in_channels // shrink * self.num_heads, in_channels)

    def forward(self, x):
        x = hip_ops.cast(x, hip_ops.compute_dtype(x))
        # the heads' outputs side by side ARE one Linear whose weight stacks the heads' weights (rows in head order)
        w = torch.cat([h.weight for h in self.head_linears], 0)
        b = torch.cat([h.bias for h in self.head_linears], 0)
        full = hip_ops.linear(x, w, b)
        return hip_ops.AddFn.apply(hip_ops.linear(full, self.proj_head.weight, self.proj_head.bias), x)


class SpectreBranchEncoderLayer(nn.Module):
    """x = norm1(x) + x;  x = norm2(x + dropout2(linear3(linear2(dropout(linear1(x))))))   (reference :35-89)"""

    def __init__(self, seq_length, d_model, nhead, dim_feedforward, dropout, activation):
        super().__init__()
        self.d_model = d_model
        layer_norm_eps = 1e-5
        self.dropout = nn.Dropout(dropout)
        self.mix_layer = nn.Linear(d_model, d_model)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, dim_feedforward)
        self.linear3 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model, eps=layer_norm_eps, bias=True)
        self.norm2 = nn.LayerNorm(d_model, eps=layer_norm_eps, bias=True)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        if isinstance(activation, str):
            activation = _get_activation_fn(activation)
        self.activation = activation   # resolved and never called, as in the reference

    def forward(self, src):
        x = hip_ops.cast(src, hip_ops.compute_dtype(src))
        x = hip_ops.add_layernorm(x, x, self.norm1.weight, self.norm1.bias, 0)   # norm1(x) + x
        h = hip_ops.dropout(hip_ops.linear(x, self.linear1.weight, self.linear1.bias), self.dropout.p, self.training)
        h = hip_ops.linear(h, self.linear2.weight, self.linear2.bias)
        f = hip_ops.dropout(hip_ops.linear(h, self.linear3.weight, self.linear3.bias), self.dropout2.p, self.training)
        return hip_ops.add_layernorm(f, x, self.norm2.weight, self.norm2.bias, 1)   # norm2(x + f)


class SpectreBranchEncoder(nn.Module):
    """out_i = spectre_project[i](cat([layer_i(out_{i-1}), feats[i]], -1));  return out_L + src   (reference :92-119)"""

    __constants__ = ["norm"]

    def __init__(self, encoder_layer, num_patches: int, num_layers: int, norm=None, reduction=1) -> None:
        if encoder_layer.d_model != 768:
            raise ValueError(f"SpectreBranchEncoder: d_model={encoder_layer.d_model}, but the reference hard-codes "
                             "Linear(768 * 2, 768) for spectre_project (spectre_branch.py:105)")
        if norm is not None:
            raise NotImplementedError("SpectreBranchEncoder: a final norm is never set by the reference (spectre_branch.py:209)")
        super().__init__()
        self.layers = _get_clones(encoder_layer, num_layers)
        self.num_layers = num_layers
        self.norm = norm
        self.spectre_branch = SpectreFeatExtractor(3, encoder_layer.d_model, num_patches, reduction=1, num_stages=num_layers)
        self.spectre_project = nn.ModuleList([nn.Linear(768 * 2, 768) for _ in range(num_layers)])

    def forward(self, src: torch.Tensor, img: torch.Tensor):
        src = hip_ops.cast(src, hip_ops.compute_dtype(src))
        _, feats = self.spectre_branch(img)
        out = src
        last = len(self.layers) - 1
        for idx, mod in enumerate(self.layers):
            proj = self.spectre_project[idx]
            # the global residual `output + src` (:119) folds into the last projection's output
            out = branch_ops.branch_project(mod(out), feats[idx], proj.weight, proj.bias, src if idx == last else None)
        return out


class SpectreFeatExtractor(nn.Module):
    """x = log1p(|rfft2(img)|); per stage k: x = Conv2d(c, 3c, 3)(x), feats[k] = pool_T(Conv2d(3c, E, 1)(x)) as (B, T, E)
    (reference :122-173).  Runs as one autograd node (branch_ops.BranchFeatFn): the 1x1 projection is applied to the pooled map
    (exact: pooling and a per-position affine map commute), and the image receives no gradient."""

    def __init__(self, in_channels, embed_dim, num_tokens, reduction=1, num_stages=1) -> None:
        if reduction != 1:
            raise NotImplementedError("SpectreFeatExtractor: reduction > 1 crops with the height and width names swapped "
                                      "(spectre_branch.py:161-164) and is never set by the reference's encoder (:102); not built")
        super().__init__()
        self.reduction = reduction
        self.num_tokens = num_tokens
        self.net = nn.ModuleList([])
        prev_channels = in_channels
        channel_scale = 3
        for _ in range(num_stages):
            self.net.append(nn.Sequential(nn.Conv2d(prev_channels, prev_channels * channel_scale, 3, stride=1)))
            prev_channels *= channel_scale
        self.project = nn.ModuleList([])
        prev_channels = in_channels * channel_scale
        for _ in range(num_stages):
            self.project.append(nn.Sequential(nn.Conv2d(prev_channels, embed_dim, 1, stride=1), nn.Flatten(start_dim=2),
                                              nn.AdaptiveAvgPool1d(num_tokens), Transpose((-2, -1))))
            prev_channels *= channel_scale

    def forward(self, x):
        if x.dtype != torch.float32:
            raise TypeError(f"SpectreFeatExtractor takes fp32 (B, C, H, W) images, got {x.dtype}")
        H, Wf = x.shape[-2], x.shape[-1] // 2 + 1
        if min(H, Wf) - 2 * len(self.net) < 1:
            raise ValueError(f"SpectreFeatExtractor: {len(self.net)} valid 3x3 stages empty the {H}x{Wf} spectrum of a "
                             f"{H}x{x.shape[-1]} image (spectre_branch.py:130-137)")
        convs = [(s[0].weight, s[0].bias) for s in self.net]
        projs = [(p[0].weight, p[0].bias) for p in self.project]
        return branch_ops.branch_features(x, convs, projs, self.num_tokens, hip_ops.compute_dtype(x))


class SpectreBranch(nn.Module):
    """reference :176-224"""

    def __init__(self, img_size=32, patch_size=4, in_channels=3, num_classes=10, embed_dim=768, num_encoders=12, num_heads=12,
                 hidden_dim=3072, dropout=0.1, activation="gelu", method="attention"):
        if embed_dim != 768:
            raise ValueError(f"SpectreBranch: embed_dim={embed_dim}, but the reference hard-codes Linear(768 * 2, 768) "
                             "(spectre_branch.py:105)")
        if in_channels != 3:
            raise ValueError(f"SpectreBranch: in_channels={in_channels}, but the reference builds the spectral branch for 3 "
                             "channels (spectre_branch.py:102)")
        wf = img_size // 2 + 1
        if min(img_size, wf) - 2 * num_encoders < 1:
            raise ValueError(f"SpectreBranch: num_encoders={num_encoders} conv stages empty the {img_size}x{wf} spectrum of a "
                             f"{img_size}x{img_size} image (each valid 3x3 stage removes 2 rows and 2 columns; at most "
                             f"{(min(img_size, wf) - 1) // 2} stages; spectre_branch.py:130-137, :213-215)")
        super().__init__()
        num_patches = (img_size // patch_size) ** 2
        self.embeddings_block = PatchEmbedding(embed_dim, patch_size, num_patches, dropout, in_channels)
        encoder_layer = SpectreBranchEncoderLayer(seq_length=num_patches + 1, d_model=embed_dim, nhead=num_heads,
                                                  dim_feedforward=hidden_dim, dropout=dropout, activation=activation)
        self.encoder_blocks = SpectreBranchEncoder(encoder_layer, num_patches + 1, num_layers=num_encoders)
        self.mlp_head = nn.Sequential(nn.Linear(embed_dim, num_classes))

    def forward(self, x, return_features=False):
        img = x
        x = self.embeddings_block(x)
        x = self.encoder_blocks(x, img)
        cls_token = x[:, 0, :]
        head = self.mlp_head[0]
        dt = hip_ops.compute_dtype(cls_token)
        if dt == torch.bfloat16 and (head.in_features % 8 or head.out_features % 8):
            dt = torch.float32   # e.g. the 100-class head: bf16 rows are not 16-byte multiples
        logits = hip_ops.linear(hip_ops.cast(cls_token.contiguous(), dt), head.weight, head.bias, True)
        if return_features:
            return logits, cls_token
        return logits
