"""Token mixers with the (B, N, D) -> (B, N, D) ``mix_layer`` contract.

The reference names them in SpectreEncoderLayer's docstring (spectre_vit/models/spectre/spectre.py:29-35:
fft_bare, dwt_embed, dwt_token, attention) but wires none of them at HEAD; BASELINE.json's configs 2-4 ask for the
parameter-free spectral ones.  SelfAttentionMixer is the control they are compared against.
"""
import torch
import torch.nn as nn

from spectre_vit import hip_ops


class FNetMixer(nn.Module):
    """y = Re(fft2(x)) over (tokens, dim), un-normalised (reference spectre_branch.py:79, orthogonal_permut.py:23-28)."""

    def forward(self, x):
        return hip_ops.FNetMixFn.apply(hip_ops.cast(x, hip_ops.compute_dtype(x)))


class HadamardMixer(nn.Module):
    """y = crop_{N,D}(H_Np . pad_{Np,Dp}(x) . H_Dp) . s over (tokens, dim): the natural-order Walsh-Hadamard transform along both axes,
    each zero-padded at its end to the next power of two and cropped back (reference spectre_vit/models/spectre/hadamar.py: fwht
    :12-32 on dim -1 then dim -2, LearnableHadamard's pad / crop :130-139).  normalize=True (fwht's default): s = (Np Dp)^-1/2.
    No parameters; the operator is symmetric, so its backward is the same kernel."""

    def __init__(self, normalize: bool = True):
        super().__init__()
        self.normalize = bool(normalize)

    def forward(self, x):
        return hip_ops.HadamardMixFn.apply(hip_ops.cast(x, hip_ops.compute_dtype(x)), self.normalize)

    def extra_repr(self):
        return f"normalize={self.normalize}"


class GlobalFilterMixer(nn.Module):
    """The learnable frequency-domain filter along the token axis (GFNet's global filter).  For x (B, N, D), N = seq_length tokens
    (the CLS row included) and K = N // 2 + 1:

        X = rfft(x, dim=1, norm="ortho")               (B, K, D) complex
        y = irfft(X * W, n=N, dim=1, norm="ortho")     (B, N, D) real

    W = view_as_complex(complex_weight); complex_weight is a float32 parameter of shape (K, D, 2), drawn as 0.02 * randn at
    construction and kept in float32 under autocast.  The operator is a depthwise circular convolution of every embedding column.
    irfft ignores the imaginary part of the DC bin and, for even N, of the Nyquist bin: y does not depend on those entries and their
    gradient is exactly zero.  The DFT table of a token count is built once per device (hip_ops.gfilter_tables)."""

    def __init__(self, seq_length: int, d_model: int):
        super().__init__()
        if seq_length < 1 or d_model < 1:
            raise ValueError(f"GlobalFilterMixer: seq_length={seq_length} and d_model={d_model} must be positive")
        self.seq_length = int(seq_length)
        self.d_model = int(d_model)
        self.complex_weight = nn.Parameter(0.02 * torch.randn(self.seq_length // 2 + 1, self.d_model, 2, dtype=torch.float32))

    def forward(self, x):
        x = hip_ops.cast(x, hip_ops.compute_dtype(x))
        if x.dim() != 3 or x.shape[1] != self.seq_length or x.shape[2] != self.d_model:
            raise ValueError(f"GlobalFilterMixer({self.seq_length}, {self.d_model}): got x of shape {tuple(x.shape)}")
        return hip_ops.GlobalFilterFn.apply(x, self.complex_weight, hip_ops.gfilter_tables(self.seq_length, x.device))

    def extra_repr(self):
        return f"seq_length={self.seq_length}, d_model={self.d_model}"


class HaarDWTMixer(nn.Module):
    """J-level Haar DWT along dim ('dwt_embed') or tokens ('dwt_token'); output bands [a_J | d_J | ... | d_1] (pywt.wavedec's order)
    in place of the transformed axis, pairs a = (x0 + x1) / sqrt2, d = (x0 - x1) / sqrt2 (PyWavelets' documented 'haar').
    PARITY UNPINNED against the reference (no model code there, only repl/dwt_experiments.py:56).

    mode: what happens to the unpaired last element of an odd length (65 tokens).  "passthrough" (default): copied into the
    approximation band -- orthonormal.  "zero": pywt's mode="zero", the convention of the reference's call: paired with a zero, so
    a_last = d_last = x_last / sqrt2; pywt would return 33 + 33 = 66 coefficients for 65 tokens -- the mixer keeps the 33
    approximation and the first 32 detail coefficients (the dropped one is a copy of a_last).  Even lengths: the modes coincide."""

    def __init__(self, axis: str = "embed", levels: int = 1, mode: str = "passthrough"):
        super().__init__()
        assert axis in ("embed", "token")
        if mode not in ("passthrough", "zero"):
            raise ValueError(f"HaarDWTMixer mode must be 'passthrough' or 'zero', got {mode!r}")
        self.axis = axis
        self.levels = levels
        self.mode = mode

    def forward(self, x):
        x = hip_ops.cast(x, hip_ops.compute_dtype(x))
        return hip_ops.HaarDWTFn.apply(x, 2 if self.axis == "embed" else 1, self.levels, self.mode == "zero")


class SelfAttentionMixer(nn.Module):
    """Self-attention over the token axis ("Native ViT Self-Attention", reference spectre.py:29-35): the arithmetic of
    ``nn.MultiheadAttention(d_model, nhead, dropout=dropout, bias=True, batch_first=True)(x, x, x, need_weights=False)[0]`` --
    no mask, scale 1/sqrt(d_model / nhead), every row (the CLS row included) attends to every row, dropout on the attention
    probabilities in training.  Parameters carry nn.MultiheadAttention's names, shapes, init and RNG order (in_proj_weight,
    in_proj_bias, out_proj.weight, out_proj.bias), so a state_dict loads strictly into either module."""

    def __init__(self, d_model: int, nhead: int, dropout: float = 0.0):
        super().__init__()
        if nhead <= 0 or d_model % nhead:
            raise ValueError(f"SelfAttentionMixer: nhead={nhead} must divide d_model={d_model}")
        self.embed_dim = d_model
        self.num_heads = nhead
        self.head_dim = d_model // nhead
        self.dropout = float(dropout)
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d_model, d_model))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * d_model))
        self.out_proj = nn.Linear(d_model, d_model)   # its weight and bias draws come first, as in nn.MultiheadAttention.__init__
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.in_proj_bias)
        nn.init.zeros_(self.out_proj.bias)

    def _p(self):
        return self.dropout if self.training else 0.0

    def forward(self, x):
        x = hip_ops.cast(x, hip_ops.compute_dtype(x))
        qkv = hip_ops.linear(x, self.in_proj_weight, self.in_proj_bias)   # packed [B, N, 3E] = q | k | v
        ctx = hip_ops.AttentionFn.apply(qkv, self.num_heads, self._p())
        return hip_ops.linear(ctx, self.out_proj.weight, self.out_proj.bias)

    def forward_cls(self, x):
        """(row 0 of forward(x), x[:, 0, :]), each (B, E): K and V over every row, Q, the attention and the out-projection at the CLS
        rows only (hip_ops.AttnClsFn; x in the compute dtype)"""
        ctx0, x0 = hip_ops.AttnClsFn.apply(x, self.in_proj_weight, self.in_proj_bias, self.num_heads, self._p())
        return hip_ops.linear(ctx0, self.out_proj.weight, self.out_proj.bias), x0

    def extra_repr(self):
        return f"embed_dim={self.embed_dim}, num_heads={self.num_heads}, dropout={self.dropout}"
