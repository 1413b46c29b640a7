"""CPU emulation of the one-product Winograd convolution (csrc/conv_f16_wx4x1.hip, VIRNET_CONV_FORM=wx4x1), stated in torch.

The arithmetic, as include/virnet_hip.h gives it for virnet_conv_wx4x1:
  weights      U[dy][j] = sum_b G[j][b] w[dy][b] in fp64; one power-of-two scale 2^e per output row that puts the row's largest |U| into
               [8192, 16384); the operand is fp16(U * 2^e), round to nearest even (the hi piece of the virnet_pack_wx4_weight image)
  activations  V_j = sum_i BT[j][i] x[4t - 1 + i] on the (pre-activated) fp32 input, in fp32 with the kernel's association
               (conv_wx4_kernel: pA / pB / pV), then ONE round to fp16 -- no lo part
  products     fp16 x fp16 is exact in fp32; the sum over 16-channel chunks and row taps is taken in fp64 here (the kernel: fp32, in MFMA order)
  epilogue     inverse scale, A^T, bias (and whatever the caller adds: mask, residual, SFT, activation) in fp32

What the emulation does not reproduce: the order of the fp32 additions inside the MFMA, fused multiply-adds the compiler forms in the
transform, and the halo rows' coefficient form -- each moves a V value by an fp32 ulp, which flips an fp16 rounding now and then
(tests/test_conv_wx4x1_gpu.py: bar A)."""
import torch
import torch.nn.functional as F

G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                 dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float32)


def weight_operand(w: torch.Tensor):
    """OIHW fp32 weight -> (fp16(U * 2^e) as float64 [co][ci][3 dy][6 positions], inverse scales 2^-e as float32 [co])."""
    u = torch.einsum("jb,okdb->okdj", G, w.double())
    m = u.float().abs().amax(dim=(1, 2, 3))
    _, ex = torch.frexp(m)
    e = torch.where(m > 0, 14 - ex, torch.zeros_like(ex)).clamp(-100, 100)
    us = torch.ldexp(u, e.view(-1, 1, 1, 1)).float().to(torch.float16).double()
    return us, torch.ldexp(torch.ones_like(m), -e)


def input_transform(x: torch.Tensor) -> torch.Tensor:
    """fp32 NCHW (already pre-activated) -> V in fp32 [n][c][h + 2][x-tiles][6], rows and columns beyond the image zero."""
    n, c, h, w = x.shape
    wp = -(-w // 4) * 4
    d = F.pad(x, (1, 1 + wp - w, 1, 1)).unfold(3, 6, 4)
    d0, d1, d2, d3, d4, d5 = (d[..., i] for i in range(6))
    a12, b12 = d4 - 4.0 * d2, d3 - 4.0 * d1
    a34, b34 = d4 - d2, d3 - d1
    return torch.stack([(4.0 * d0 + d4) - 5.0 * d2, a12 + b12, a12 - b12, a34 + 2.0 * b34, a34 - 2.0 * b34, (4.0 * d1 + d5) - 5.0 * d3], dim=-1)


def conv_wx4x1(x: torch.Tensor, w: torch.Tensor, b=None) -> torch.Tensor:
    """The stride-1 3x3 'same' convolution of fp32 NCHW ``x`` (already pre-activated) with OIHW ``w`` in the one-product arithmetic -> fp32 NCHW."""
    n, c, h, wd = x.shape
    us, inv = weight_operand(w)
    vh = input_transform(x.float()).to(torch.float16).double()
    m = sum(torch.einsum("ocj,nchtj->nohtj", us[:, :, dy, :], vh[:, :, dy:dy + h]) for dy in range(3))
    y = torch.einsum("kj,nohtj->nohtk", AT, m.float()) * inv.view(1, -1, 1, 1, 1)
    y = y.reshape(n, w.shape[0], h, -1)[..., :wd]
    return y if b is None else y + b.float().view(1, -1, 1, 1)


def conv_bf16_operands(x: torch.Tensor, w: torch.Tensor, b=None) -> torch.Tensor:
    """fp64 convolution of bf16-rounded operands (what a one-product bf16 direct kernel computes, up to summation order) -> fp64 NCHW."""
    y = F.conv2d(x.float().to(torch.bfloat16).double(), w.float().to(torch.bfloat16).double(), None, padding=1)
    return y if b is None else y + b.double().view(1, -1, 1, 1)


# ---- the layer cases of tests/test_conv_wx4x1_gpu.py: (channels, h, w, n), pre-activation 0.2 + residual + dual store -----------------
SHAPES = [(64, 9, 33, 2), (96, 17, 70, 1), (192, 6, 31, 2), (288, 16, 64, 1), (160, 18, 40, 1), (224, 33, 31, 1), (32, 3, 2, 1), (96, 40, 64, 4)]


def three_errors(xa: torch.Tensor, w: torch.Tensor, b: torch.Tensor, post=lambda y: y):
    """(fp64 reference, emulation, e_m, e_b) of one conv on the pre-activated fp32 input ``xa``; ``post``: the epilogue (mask, residual,
    ...), applied alike to the fp64 reference, the emulation and the bf16-operand conv.
      e_m = max |emulation - fp64|        e_b = max |fp64 conv of bf16-rounded operands - fp64|"""
    ref = post(F.conv2d(xa.double(), w.double(), b.double(), padding=1))
    emu = post(conv_wx4x1(xa, w, b))
    e_m = float((emu.double() - ref).abs().max())
    e_b = float((post(conv_bf16_operands(xa, w, b)) - ref).abs().max())
    return ref, emu, e_m, e_b
