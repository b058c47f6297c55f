"""Network spec + weight-file format shared by the oracle, the HIP engine and the tests.

The reference ships no network (its UNet lives in an unpublished TensorRT engine,
/root/reference/src/initialize.cpp:49-60, .gitignore:2-8).  The topology is the one
BASELINE.json names; the free choices are fixed HERE, once:

  * double conv = [conv3x3 pad1 (no bias) -> BatchNorm(eval, eps) -> ReLU] x 2
  * down_i      = maxpool 2x2 s2 -> double conv (C -> 2C)
  * up_i        = convT 2x2 s2 (C -> C/2, with bias) -> concat [skip, upsampled] on channels
                  -> double conv (C -> C/2)
  * outc        = conv1x1 (base -> classes, with bias)

The decoder has a second form, `up = "bilinear"` (Pytorch-UNet's bilinear=True), with ch[i] = base << i, L = levels and
lvl = L - i for up_i:
  * down_L      = maxpool -> double conv ch[L-1] -> ch[L-1] -> ch[L-1]   (the bottleneck is halved: Pytorch-UNet's factor 2)
  * up_i        = bilinear x2, align_corners=True (no weights, ch[lvl] channels) -> concat [skip, upsampled]
                  -> double conv 2 ch[lvl] -> ch[lvl] -> ch[lvl] / 2  (ch[0] -> ch[0] at the last level)
  * I/O contract of the reference: input  fp32 NCHW [B,in_ch,H,W] = u8/255.0f
    (src/process.cpp:22-42, :70-71), output fp32 NCHW planar logits [B,classes,H,W]
    (src/process.cpp:81-85, :163), first-max-wins argmax (src/process.cpp:158-170).

Weight file ("MIUNETW1"), little endian:
    char  magic[8] = "MIUNETW1"
    u32   version            1 = transposed decoder; 2 = the decoder named by up_mode
    u32   in_ch, base, levels, classes
    f32   bn_eps
    u32   n_floats           (payload length, for a truncation check)
    u32   up_mode            version 2 only: 0 = transposed 2x2, 1 = bilinear x2 align-corners
    f32   payload[n_floats]  tensors in `tensor_list()` order, PyTorch-native layouts:
          conv3x3 [Cout][Cin][3][3]; BN gamma,beta,mean,var [C]; convT [Cin][Cout][2][2] + bias[Cout];
          outc [classes][base] + bias[classes]
A transposed net is always written as version 1 (byte for byte what earlier releases wrote); a bilinear one as version 2.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

MAGIC = b"MIUNETW1"
HEADER = struct.Struct("<8sIIIIIfI")
UP_MODE = struct.Struct("<I")
UP_MODES = ("transpose", "bilinear")      # index = the file's up_mode


@dataclass(frozen=True)
class UNetSpec:
    in_ch: int = 1
    base: int = 64
    levels: int = 4
    classes: int = 3
    bn_eps: float = 1e-5
    up: str = "transpose"

    def __post_init__(self):
        if self.up not in UP_MODES:
            raise ValueError(f"up must be one of {UP_MODES}, not {self.up!r}")

    def channels(self):
        return [self.base << i for i in range(self.levels + 1)]

    def widths(self):
        """[(prefix, cin, mid, cout)] of every double conv, in file order."""
        ch, L = self.channels(), self.levels
        out = [("inc", self.in_ch, ch[0], ch[0])]
        for i in range(1, L + 1):
            c = ch[i - 1] if (i == L and self.up == "bilinear") else ch[i]
            out.append((f"down{i}", ch[i - 1], c, c))
        for i in range(1, L + 1):
            c = ch[L - i]
            if self.up == "bilinear":
                out.append((f"up{i}", 2 * c, c, c // 2 if L - i > 0 else c))
            else:
                out.append((f"up{i}", 2 * c, c, c))
        return out

    def tensor_list(self):
        """[(name, shape)] in file order."""
        out = []

        for prefix, cin, mid, cout in self.widths():
            if prefix.startswith("up") and self.up == "transpose":
                out.append((f"{prefix}.t.w", (cin, cin // 2, 2, 2)))
                out.append((f"{prefix}.t.b", (cin // 2,)))
            for k, ci, co in ((1, cin, mid), (2, mid, cout)):
                out.append((f"{prefix}.c{k}.w", (co, ci, 3, 3)))
                for n in ("gamma", "beta", "mean", "var"):
                    out.append((f"{prefix}.bn{k}.{n}", (co,)))
        ch = self.channels()
        out.append(("outc.w", (self.classes, ch[0])))
        out.append(("outc.b", (self.classes,)))
        return out

    def n_params(self):
        return int(sum(int(np.prod(s)) for _, s in self.tensor_list()))

    def macs_per_image(self, h, w):
        """Algorithmic MACs: conv3x3 = H*W*Cin*Cout*9, convT = Hout*Wout*Cin*Cout, 1x1 = H*W*Cin*Cout;
        the bilinear upsample counts 0."""
        m = 0
        L = self.levels
        for k, (prefix, cin, mid, cout) in enumerate(self.widths()):
            lvl = k if k <= L else 2 * L - k          # inc, down1..downL, then up1 (level L-1) .. upL (level 0)
            px = (h >> lvl) * (w >> lvl)
            m += px * 9 * (cin * mid + mid * cout)
            if prefix.startswith("up") and self.up == "transpose":
                m += px * cin * (cin // 2)
        m += h * w * self.channels()[0] * self.classes
        return m


def pack_weights(spec: UNetSpec, tensors: dict) -> bytes:
    parts = []
    for name, shape in spec.tensor_list():
        t = np.ascontiguousarray(tensors[name], dtype=np.float32)
        if t.shape != tuple(shape):
            raise ValueError(f"{name}: shape {t.shape} != {shape}")
        parts.append(t.reshape(-1))
    payload = np.concatenate(parts)
    if spec.up == "transpose":
        hdr = HEADER.pack(MAGIC, 1, spec.in_ch, spec.base, spec.levels, spec.classes, spec.bn_eps, payload.size)
    else:
        hdr = HEADER.pack(MAGIC, 2, spec.in_ch, spec.base, spec.levels, spec.classes, spec.bn_eps, payload.size)
        hdr += UP_MODE.pack(UP_MODES.index(spec.up))
    return hdr + payload.tobytes()


def unpack_weights(blob: bytes):
    magic, ver, in_ch, base, levels, classes, eps, n = HEADER.unpack_from(blob, 0)
    if magic != MAGIC:
        raise ValueError("not a MIUNETW1 weight file")
    if ver == 1:
        up, off = "transpose", HEADER.size
    elif ver == 2:
        (mode,) = UP_MODE.unpack_from(blob, HEADER.size)
        if mode >= len(UP_MODES):
            raise ValueError(f"unknown up_mode {mode} in a version 2 weight file")
        up, off = UP_MODES[mode], HEADER.size + UP_MODE.size
    else:
        raise ValueError(f"unsupported MIUNETW1 version {ver}")
    spec = UNetSpec(in_ch, base, levels, classes, eps, up)
    if len(blob) < off + 4 * n:
        raise ValueError("weight file truncated: shorter than its payload length")
    payload = np.frombuffer(blob, dtype="<f4", count=n, offset=off)
    if n != spec.n_params():
        raise ValueError("payload length does not match the header's topology")
    tensors = {}
    off = 0
    for name, shape in spec.tensor_list():
        k = int(np.prod(shape))
        tensors[name] = payload[off:off + k].reshape(shape)
        off += k
    return spec, tensors
