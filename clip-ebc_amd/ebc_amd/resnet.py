"""CLIP-EBC with the CLIP ResNet-50 backbone (config 2: clip_resnet50, 448 crops, reduction 8, bf16).

Reference surface:
  * image encoder `ModifiedResNet(features_only=True, out_indices=(-1,), reduction)` with its stem, the
    anti-aliased Bottleneck stages and layer4 at stride 1 when reduction <= 16 (models/clip/_clip/
    image_encoder.py:10-115, blocks.py:56-101).  It is TRAINABLE for the ResNet backbones
    (models/clip/model.py:51-52: no freezing) and runs on PyTorch-ROCm (MIOpen convolutions, channels_last,
    the caller's autocast) -- SURVEY.md §8 keeps the encoder off the HIP path for this config.
  * decoder `Bottleneck(2048, 2048, expansion=1)` (models/utils.py:306-363, cfg [2048] from
    models/clip/model.py:234-238, `_init_weights` :366-379) and the projection + similarity head: on
    libebc_hip.so (`_BottleneckFn`, `model._HeadFn` at embed width 1024).

Layout on the HIP side: the encoder's NHWC (channels_last) layer4 output is taken as f32 rows
[B, h, w, 2048]; every decoder activation is an unpadded row matrix [P = B*H*W][2048] in the compute dtype,
except conv2's input, which is the zero-padded image the implicit-GEMM 3x3 conv reads.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from ._blocks import (_conv1x1_bwd, _conv1x1_fwd, _conv3x3_bwd, _conv3x3_fwd, _dec_workspace, _geometry, _prep_1x1,
                      _prep_3x3)


# ----------------------------------------------------------------------------- encoder (PyTorch-ROCm)
class AttnBottleneck(nn.Module):
    """blocks.py:56-101: 1x1 -> 3x3 -> avgpool(stride) -> 1x1 (x4), downsample = avgpool + 1x1 + BN."""
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu2 = nn.ReLU(inplace=True)
        self.avgpool = nn.AvgPool2d(stride) if stride > 1 else nn.Identity()
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu3 = nn.ReLU(inplace=True)
        self.downsample = None
        self.stride = stride
        if stride > 1 or inplanes != planes * self.expansion:
            self.downsample = nn.Sequential(OrderedDict([
                ("-1", nn.AvgPool2d(stride)),
                ("0", nn.Conv2d(inplanes, planes * self.expansion, 1, stride=1, bias=False)),
                ("1", nn.BatchNorm2d(planes * self.expansion))]))

    def forward(self, x: Tensor) -> Tensor:
        out = self.relu1(self.bn1(self.conv1(x)))
        out = self.relu2(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(self.avgpool(out)))
        idt = x if self.downsample is None else self.downsample(x)
        return self.relu3(out + idt)


class ModifiedResNet(nn.Module):
    """image_encoder.py:10-115 with features_only=True, out_indices=(-1,): returns layer4's output."""

    def __init__(self, layers: Tuple[int, int, int, int] = (3, 4, 6, 3), output_dim: int = 1024,
                 input_resolution: int = 224, width: int = 64, heads: int = 32, reduction: Optional[int] = 32,
                 **kw: Any) -> None:
        super().__init__()
        reduction = 32 if reduction is None else reduction
        self.input_resolution = (input_resolution, input_resolution)
        self.downsampling_rate = 32
        self.conv1 = nn.Conv2d(3, width // 2, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width // 2)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(width // 2, width // 2, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width // 2)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv3 = nn.Conv2d(width // 2, width, 3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(width)
        self.relu3 = nn.ReLU(inplace=True)
        self.avgpool = nn.AvgPool2d(2)
        self._inplanes = width
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(width * 8, layers[3], stride=1 if reduction <= 16 else 2)
        self.features_only, self.out_indices = True, [4]
        self.channels = width * 32
        self.reduction = self.downsampling_rate // 2 if reduction <= 16 else self.downsampling_rate
        self.clip_embed_dim = output_dim

    def _make_layer(self, planes: int, blocks: int, stride: int = 1) -> nn.Sequential:
        layers = [AttnBottleneck(self._inplanes, planes, stride)]
        self._inplanes = planes * AttnBottleneck.expansion
        for _ in range(1, blocks):
            layers.append(AttnBottleneck(self._inplanes, planes))
        return nn.Sequential(*layers)

    def forward(self, x: Tensor) -> Tensor:
        x = x.type(self.conv1.weight.dtype)
        x = self.relu1(self.bn1(self.conv1(x)))
        x = self.relu2(self.bn2(self.conv2(x)))
        x = self.relu3(self.bn3(self.conv3(x)))
        x = self.avgpool(x)
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))


# ----------------------------------------------------------------------------- decoder (HIP)
class Bottleneck(nn.Module):
    """Parameter layout of models/utils.py:306-363 (ResNet v1.5 Bottleneck; the decoder uses expansion 1 and
    in_channels == out_channels, so `downsample` is the identity)."""

    def __init__(self, in_channels: int, out_channels: int, expansion: int = 1, **kw: Any) -> None:
        super().__init__()
        if expansion != 1 or in_channels != out_channels:
            raise NotImplementedError("decoder Bottleneck: expansion 1, in_channels == out_channels only "
                                      "(clip_resnet50's cfg [2048], models/clip/model.py:237-238)")
        w = out_channels
        self.expansion = expansion
        self.conv1 = nn.Conv2d(in_channels, w, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(w)
        self.conv2 = nn.Conv2d(w, w, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(w)
        self.conv3 = nn.Conv2d(w, out_channels, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.stride = 1
        self.downsample = nn.Identity()


def _ws(L, dev, dt, B, H, W, C, N, P, Cmax):
    """Stream-owned scratch for one block: the 3x3 conv's (split-K counters + BN partials) and the flat BN kernels'
    column partials over P rows of up to Cmax channels."""
    rpb = 8 * max(1, 512 // max(1, Cmax // 8))
    need = max(L.ebc_dec_workspace_bytes(dt, B, H, W, C, N), 16384 + (-(-P // rpb)) * 8 * Cmax)
    return _dec_workspace(dev, need)


class _ResBlockFn(torch.autograd.Function):
    """One ModifiedResNet Bottleneck (blocks.py:56-101) on libebc_hip.so, NHWC rows in the compute dtype:
    conv1 1x1 -> bn1 -> relu -> conv2 3x3 -> bn2 -> relu -> avgpool(stride) -> conv3 1x1 -> bn3 (+ identity:
    x, or avgpool(stride) -> 1x1 -> bn for the downsample branch) -> relu.  x [B,H,W,Cin] -> y [B,H/s,W/s,4p]."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, wd, g1, b1, g2, b2, g3, b3, gd, bd, blk, cdtype, training):
        with _lib.on(x):
            return _ResBlockFn._forward(ctx, x, (w1, w2, w3, wd), blk, cdtype, training)

    @staticmethod
    def _forward(ctx, x, wts, blk, cdtype, training):
        L = _lib.lib()
        x = x.detach()
        if x.dtype != cdtype or not x.is_contiguous():
            x = x.to(cdtype).contiguous()
        B, H, W, Cin = x.shape
        s = blk.stride
        Ho, Wo = H // s, W // s
        P, Po = B * H * W, B * Ho * Wo
        planes, Cout = wts[0].shape[0], wts[2].shape[0]
        down = blk.downsample is not None
        dev, dt, st = x.device, _lib.dtype_code(cdtype), _lib.stream(x)
        ws = _ws(L, dev, dt, B, H, W, planes, planes, P, max(Cin, Cout, planes))
        geo = _geometry(L, dt, B, H, W, planes, planes)
        W1, W1t = _prep_1x1(L, wts[0], cdtype, st)
        W3, W3t = _prep_1x1(L, wts[2], cdtype, st)
        Wd, Wdt = _prep_1x1(L, wts[3], cdtype, st) if down else (None, None)
        wk2, wf2 = _prep_3x3(L, wts[1], cdtype, st)
        # conv1 1x1 -> bn1 -> relu1, into the zero-padded conv2 input
        s1 = _conv1x1_fwd(L, blk.bn1, x.view(P, Cin), W1, training, dt, ws, st)
        h1pad = torch.empty(geo.Q, planes, device=dev, dtype=cdtype)
        _lib.check(L.ebc_bn_relu_pad(dt, _lib.ptr(s1.z), _lib.ptr(s1.scale), _lib.ptr(s1.shift), _lib.ptr(h1pad), B, H, W,
                                     planes, st), "ebc_bn_relu_pad")
        # conv2 3x3 (BN statistics in the epilogue) -> bn2 -> relu2 -> avgpool(stride)
        s2 = _conv3x3_fwd(L, blk.bn2, h1pad, wk2, geo, training, dt, ws, st)
        h2p = torch.empty(Po, planes, device=dev, dtype=cdtype)
        if s > 1:
            _lib.check(L.ebc_bn_relu_avgpool(dt, _lib.ptr(s2.z), _lib.ptr(s2.scale), _lib.ptr(s2.shift), _lib.ptr(h2p),
                                             B, H, W, planes, st), "ebc_bn_relu_avgpool")
        else:
            _lib.check(L.ebc_bn_relu(dt, _lib.ptr(s2.z), _lib.ptr(s2.scale), _lib.ptr(s2.shift), _lib.ptr(h2p), P, planes,
                                     st), "ebc_bn_relu")
        # conv3 1x1 -> bn3
        s3 = _conv1x1_fwd(L, blk.bn3, h2p, W3, training, dt, ws, st)
        # identity: x, or avgpool(stride) -> 1x1 -> bn (downsample "-1", "0", "1")
        xd = sd = None
        if down:
            if s > 1:
                xd = torch.empty(Po, Cin, device=dev, dtype=cdtype)
                _lib.check(L.ebc_avgpool2(dt, dt, _lib.ptr(x), _lib.ptr(xd), B, H, W, Cin, st), "ebc_avgpool2")
            else:
                xd = x.view(P, Cin)
            sd = _conv1x1_fwd(L, blk.downsample[2], xd, Wd, training, dt, ws, st)
        y = torch.empty(B, Ho, Wo, Cout, device=dev, dtype=cdtype)
        _lib.check(L.ebc_bn_add_relu_flat(dt, _lib.ptr(s3.z), _lib.ptr(s3.scale), _lib.ptr(s3.shift),
                                          _lib.ptr(sd.z if down else x), _lib.ptr(sd.scale) if down else None,
                                          _lib.ptr(sd.shift) if down else None, _lib.ptr(y), Po, Cout, st),
                   "ebc_bn_add_relu_flat")
        ctx.save_for_backward(x, h1pad, h2p, y, W1t, wf2, W3t, *((xd, Wdt) if down else ()))
        ctx.states = (s1, s2, s3, sd)
        ctx.gammas = (blk.bn1.weight, blk.bn2.weight, blk.bn3.weight, blk.downsample[2].weight if down else None)
        ctx.geo = geo
        ctx.meta = (Cin, s, Po, Cout, down, cdtype, x.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        with _lib.on(gy):
            return _ResBlockFn._backward(ctx, gy)

    @staticmethod
    def _backward(ctx, gy):
        L = _lib.lib()
        Cin, s, Po, Cout, down, cdtype, xdt = ctx.meta
        geo = ctx.geo
        B, H, W, planes, P = geo.B, geo.H, geo.W, geo.C, geo.P
        saved = ctx.saved_tensors
        x, h1pad, h2p, y, W1t, wf2, W3t = saved[:7]
        xd, Wdt = saved[7:] if down else (None, None)
        s1, s2, s3, sd = ctx.states
        g1, g2, g3, gd = ctx.gammas
        dev, dt, st = y.device, _lib.dtype_code(cdtype), _lib.stream(y)
        gy = gy.to(cdtype).contiguous().view(Po, Cout)
        ws = _ws(L, dev, dt, B, H, W, planes, planes, P, max(Cin, Cout, planes))
        f32 = dict(device=dev, dtype=torch.float32)
        # bn3 (+ relu3 through y) -> conv3; without a downsample the identity's gradient is g = gy * (y > 0) itself (f32)
        gid = None if down else torch.empty(Po, Cout, **f32)
        dh2p, dw3, dg3, db3 = _conv1x1_bwd(L, s3, g3, gy, y, h2p, W3t, dt, ws, st, gmask=gid)
        dwd = dgd = dbd = None
        if down:
            # downsample bn (same masked gradient) -> 1x1 -> avgpool: the identity's input gradient, f32
            dxd, dwd, dgd, dbd = _conv1x1_bwd(L, sd, gd, gy, y, xd, Wdt, dt, ws, st, out_f32=True)
            if s > 1:
                gid = torch.empty(P, Cin, **f32)
                _lib.check(L.ebc_avgpool2_bwd(_lib.EBC_F32, _lib.EBC_F32, _lib.ptr(dxd), _lib.ptr(gid), B, H, W, Cin, st),
                           "ebc_avgpool2_bwd(downsample)")
                del dxd
            else:
                gid = dxd
        # avgpool -> relu2 -> bn2 (ReLU mask recomputed from z2) -> conv2's gradients
        if s > 1:
            dh2 = torch.empty(P, planes, device=dev, dtype=cdtype)
            _lib.check(L.ebc_avgpool2_bwd(dt, dt, _lib.ptr(dh2p), _lib.ptr(dh2), B, H, W, planes, st), "ebc_avgpool2_bwd")
            del dh2p
        else:
            dh2 = dh2p
        dh1, dw2, dg2, db2 = _conv3x3_bwd(L, s2, g2, dh2, None, h1pad, wf2, geo, dt, ws, ws, st)
        del dh2
        # bn1 (ReLU mask recomputed from z1) -> conv1: dx = dz1 W1 + the identity's gradient
        dx, dw1, dg1, db1 = _conv1x1_bwd(L, s1, g1, dh1, None, x.view(P, Cin), W1t, dt, ws, st, resid=gid)
        dx = dx.view(B, H, W, Cin)
        ctx.states = None
        return (dx.to(xdt) if xdt != cdtype else dx, dw1.view(planes, Cin, 1, 1), dw2, dw3.view(Cout, planes, 1, 1),
                None if dwd is None else dwd.view(Cout, Cin, 1, 1), dg1, db1, dg2, db2, dg3, db3, dgd, dbd,
                None, None, None)


def encoder_forward(enc: "ModifiedResNet", x: Tensor, cdtype: torch.dtype, training: bool) -> Tensor:
    """ModifiedResNet forward with the 16 Bottlenecks on libebc_hip.so: the 3-conv stem + avgpool on
    PyTorch-ROCm (3- and 32-channel convolutions), then NHWC rows through `_ResBlockFn`.
    Returns layer4's output as NHWC [B, h, w, 2048] in the compute dtype."""
    h = x.type(enc.conv1.weight.dtype).contiguous(memory_format=torch.channels_last)
    h = enc.relu1(enc.bn1(enc.conv1(h)))
    h = enc.relu2(enc.bn2(enc.conv2(h)))
    h = enc.avgpool(enc.relu3(enc.bn3(enc.conv3(h))))
    h = h.permute(0, 2, 3, 1)
    with torch.autocast("cuda", enabled=False):
        for layer in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
            for blk in layer:
                d = blk.downsample
                h = _ResBlockFn.apply(h, blk.conv1.weight, blk.conv2.weight, blk.conv3.weight,
                                      None if d is None else d[1].weight, blk.bn1.weight, blk.bn1.bias, blk.bn2.weight,
                                      blk.bn2.bias, blk.bn3.weight, blk.bn3.bias, None if d is None else d[2].weight,
                                      None if d is None else d[2].bias, blk, cdtype, training)
    return h


class _BottleneckFn(torch.autograd.Function):
    """Bottleneck(C, C, expansion=1) decoder after the x`up` bilinear adapt (models/clip/model.py:195-197;
    models/utils.py:346-363): conv1x1-BN-ReLU, conv3x3-BN-ReLU, conv1x1-BN, + x, ReLU.
    feat [B,h,w,C] f32 (NHWC) -> y [B,H,W,C] in the compute dtype."""

    @staticmethod
    def forward(ctx, feat, w1, w2, w3, g1, b1, g2, b2, g3, b3, blk, up, cdtype, training):
        with _lib.on(feat):
            return _BottleneckFn._forward(ctx, feat, (w1, w2, w3), (g1, g2, g3), blk, up, cdtype, training)

    @staticmethod
    def _forward(ctx, feat, wts, gammas, blk, up, cdtype, training):
        L = _lib.lib()
        feat = feat.detach().contiguous()
        B, h, w, C = feat.shape
        H, W = h * up, w * up
        N = wts[0].shape[0]
        if N != C or C % 256:
            raise NotImplementedError("fused Bottleneck decoder: C == N, C % 256 == 0")
        dev, dt, st = feat.device, _lib.dtype_code(cdtype), _lib.stream(feat)
        geo = _geometry(L, dt, B, H, W, C, N)
        P = geo.P
        ws = _dec_workspace(dev, L.ebc_dec_workspace_bytes(dt, B, H, W, C, N))
        x = torch.empty(P, C, device=dev, dtype=cdtype)
        _lib.check(L.ebc_dec_upsample(dt, _lib.ptr(feat), _lib.ptr(x), B, h, w, C, up, st), "ebc_dec_upsample")
        W1, W1t = _prep_1x1(L, wts[0], cdtype, st)
        W3, W3t = _prep_1x1(L, wts[2], cdtype, st)
        wk2, wf2 = _prep_3x3(L, wts[1], cdtype, st)
        # conv1 (1x1) + bn1 + relu -> padded conv2 input
        s1 = _conv1x1_fwd(L, blk.bn1, x, W1, training, dt, ws, st)
        h1pad = torch.empty(geo.Q, N, device=dev, dtype=cdtype)
        _lib.check(L.ebc_bn_relu_pad(dt, _lib.ptr(s1.z), _lib.ptr(s1.scale), _lib.ptr(s1.shift), _lib.ptr(h1pad), B, H, W,
                                     N, st), "ebc_bn_relu_pad")
        # conv2 (3x3, BN statistics in the GEMM epilogue) + bn2 + relu
        s2 = _conv3x3_fwd(L, blk.bn2, h1pad, wk2, geo, training, dt, ws, st)
        h2 = torch.empty(P, N, device=dev, dtype=cdtype)
        _lib.check(L.ebc_bn_relu(dt, _lib.ptr(s2.z), _lib.ptr(s2.scale), _lib.ptr(s2.shift), _lib.ptr(h2), P, N, st),
                   "ebc_bn_relu")
        # conv3 (1x1) + bn3 + identity + relu
        s3 = _conv1x1_fwd(L, blk.bn3, h2, W3, training, dt, ws, st)
        y = torch.empty(B, H, W, N, device=dev, dtype=cdtype)
        _lib.check(L.ebc_bn_add_relu(dt, _lib.ptr(s3.z), _lib.ptr(s3.scale), _lib.ptr(s3.shift), _lib.ptr(feat), up,
                                     _lib.ptr(y), B, H, W, N, st), "ebc_bn_add_relu")
        ctx.save_for_backward(x, h1pad, h2, y, W1t, wf2, W3t, *gammas)
        ctx.states = (s1, s2, s3)
        ctx.geo = geo
        ctx.meta = (h, w, up, cdtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        with _lib.on(gy):
            return _BottleneckFn._backward(ctx, gy)

    @staticmethod
    def _backward(ctx, gy):
        L = _lib.lib()
        x, h1pad, h2, y, W1t, wf2, W3t, g1, g2, g3 = ctx.saved_tensors
        s1, s2, s3 = ctx.states
        h, w, up, cdtype = ctx.meta
        geo = ctx.geo
        B, H, W, C, N, P = geo.B, geo.H, geo.W, geo.C, geo.N, geo.P
        dev, dt, st = y.device, _lib.dtype_code(cdtype), _lib.stream(y)
        gy = gy.to(cdtype).contiguous().view(P, N)
        ws = _dec_workspace(dev, L.ebc_dec_workspace_bytes(dt, B, H, W, C, N))
        # bn3 (+ relu through the block output y) -> conv3; the identity branch keeps g = gy * (y > 0) in f32
        gid = torch.empty(P, C, device=dev, dtype=torch.float32)
        dh2, dw3, dg3, db3 = _conv1x1_bwd(L, s3, g3, gy, y, h2, W3t, dt, ws, st, gmask=gid)
        # bn2 (+ relu through h2) -> conv2's gradients
        dh1, dw2, dg2, db2 = _conv3x3_bwd(L, s2, g2, dh2, h2, h1pad, wf2, geo, dt, ws, ws, st)
        del dh2
        # bn1 (ReLU mask recomputed from z1) -> conv1: dx = dz1 W1 + the identity branch's gradient (f32, in place over gid)
        _, dw1, dg1, db1 = _conv1x1_bwd(L, s1, g1, dh1, None, x, W1t, dt, ws, st, resid=gid, out=gid, out_f32=True)
        dfeat = torch.empty(B, h, w, C, device=dev, dtype=torch.float32)
        _lib.check(L.ebc_dec_upsample_bwd(_lib.EBC_F32, _lib.ptr(gid), _lib.ptr(dfeat), B, h, w, C, up, st),
                   "ebc_dec_upsample_bwd")
        ctx.states = None
        return (dfeat, dw1.view(N, C, 1, 1), dw2, dw3.view(N, N, 1, 1), dg1, db1, dg2, db2, dg3, db3,
                None, None, None, None)
