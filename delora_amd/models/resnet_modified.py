"""ResNet-18-shaped feature extractor for 360 degree range images (reference src/models/resnet_modified.py).

Same topology and parameter names as the reference so that its checkpoints load unchanged
(``conv1``, ``layer{1..4}.{i}.conv{1,2}``, ``layer{2,3,4}.0.downsample.0``, ``fc``): no normalisation layers,
tanh (or relu) activations, every 3x3 convolution sees one wrapped column on each side of W and one zero row on
each side of H, strides (1,2) in the stem/pool/layer2/layer3 and (2,2) in layer4.

Two GPU paths compute it (``cnn_impl``; both are compared with each other and with torch-CPU in the tests):
  * fp32 tensors on shapes that tile (the reference's full-size network on 64/128-ring images, and the narrow networks of
    ``factor_fewer_resnet_channels`` 2 and 4, whose layers below 64 channels run on the narrow MFMA family, csrc/narrow.hip): three autograd
    Functions on channels-last activations -- ``ring_conv.RingStem`` (conv1 + activation + max-pooling), ``RingSegment``
    for layer1..layer4 (fused Winograd / direct MFMA convolutions with the wrap-around as addressing and the elementwise tail
    in their epilogues; one Function in a single process, cut per layer under DDP so that the gradient all-reduce overlaps
    the backward) and ``MeanHW`` before ``fc``; inside ``torch.autocast`` the same structure in bf16 / fp16
    (``RingSegmentH``: csrc/convh.hip, wgradh.hip).  ``use_dropout`` in training mode stays on this path: the input mask is applied
    inside the stem's transposing copy, the channel mask by ``ring_conv.ChannelDropout`` at an extra cut in front of layer4, the
    fc mask inside the fused heads (csrc/dropout.hip: a counter-based stream of the library's own, seeded per forward pass);
  * everything else (factor 8, narrow networks under autocast or behind the feature tower, widths that are not multiples of 4,
    ``cnn_impl: modules``): the modules below -- library convolutions on inputs that
    travel in wrapped form, with activation (+ residual add) and the wrap-around padding as ONE fused HIP elementwise op
    (``ring_ops.ring_act_pad``) instead of the reference's separate tanh, add and three-copy F.pad per layer, and the
    stem's activation + padding + max-pooling + padding as one more (``ring_ops.ring_act_pool_pad``).
"""
import torch

from . import ring_conv
from .ring_ops import ring_act_pad, ring_act_pool_pad


class RingConv2d(torch.nn.Conv2d):
    """Bias-free 3x3 convolution of a 360-degree image whose input is ALREADY wrapped by one column on each side of W
    (see ring_ops.ring_act_pad); H gets ordinary zero padding.  Parameters are those of nn.Conv2d (key
    ``<name>.weight``).  Reference: F.pad(..., (1,1,0,0), 'circular') followed by Conv2d(padding=(1,0)),
    resnet_modified.py:97-98,162-168."""

    def __init__(self, in_planes, out_planes, stride=1):
        super().__init__(in_planes, out_planes, kernel_size=3, stride=stride, padding=(1, 0), bias=False)


class BasicBlock(torch.nn.Module):
    """Two ring convolutions with a residual connection (reference resnet_modified.py:136-177).  Activations travel
    between convolutions in wrapped ("padded") form: the block takes a padded, activated input and returns a padded,
    activated output, and each of its two elementwise stages -- activation, and residual add + activation -- is fused
    with the wrap-around padding of the next convolution's input."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, activation_fct="relu"):
        super().__init__()
        self.conv1 = RingConv2d(inplanes, planes, stride=stride)
        self.conv2 = RingConv2d(planes, planes)
        self.activation = torch.nn.ReLU(inplace=True) if activation_fct == "relu" else torch.nn.Tanh()
        self.act_name = "relu" if activation_fct == "relu" else "tanh"
        self.downsample = downsample
        self.stride = stride
        self.pad_out = True             # the last block of the network returns an unpadded tensor

    def forward(self, p_in):
        p_mid = ring_act_pad(self.conv1(p_in), self.act_name, pad=True)
        v = self.conv2(p_mid)
        if self.downsample is None:
            shortcut = p_in                                         # padded tensor: its interior is the residual
        else:
            shortcut = self.downsample(p_in[..., 1:-1])             # 1x1 strided convolution of the unpadded input
        return ring_act_pad(v, self.act_name, pad=self.pad_out, residual=shortcut)


class ResNetModified(torch.nn.Module):
    def __init__(self, in_channels, num_outputs, use_dropout=False, layers=(2, 2, 2, 2),
                 factor_fewer_resnet_channels=1, activation_fct="relu", impl="auto"):
        super().__init__()
        self.activation_fct = activation_fct
        # "auto": the channels-last HIP trunk (ring_conv.RingTrunk: fp32 MFMA convolutions with fused epilogues) whenever
        # the tensors are fp32 on the GPU and the shapes tile, the module path (library convolutions + fused ring ops)
        # otherwise; "modules" forces the latter, "hip" makes unsupported shapes an error.
        self.impl = impl
        self.use_dropout = bool(use_dropout)
        # config key amp_stem (OdometryModel sets it): inside autocast the stem runs in the autocast dtype too (ring_conv.RingStemH)
        # instead of fp32 in front of the half-precision trunk.  Off by default: it rounds the range image itself to 8 / 11 bits.
        self.amp_stem = False
        self.dropout_p = 0.2                           # the reference's rate at all three sites (resnet_modified.py:33-38)
        widths = [int(c / factor_fewer_resnet_channels) for c in (64, 128, 256, 512)]
        self.inplanes = widths[0]
        self.dropout_values = torch.nn.Dropout(p=0.2) if use_dropout else torch.nn.Identity()
        self.dropout_channels = torch.nn.Dropout2d(p=0.2) if use_dropout else torch.nn.Identity()
        self.conv1 = RingConv2d(in_channels, self.inplanes, stride=(1, 2))
        self.relu = torch.nn.ReLU(inplace=True)
        self.tanh = torch.nn.Tanh()
        self.maxpool = torch.nn.MaxPool2d(kernel_size=3, stride=(1, 2), padding=(1, 0))
        self.layer1 = self._make_layer(widths[0], layers[0], stride=1)
        self.layer2 = self._make_layer(widths[1], layers[1], stride=(1, 2))
        self.layer3 = self._make_layer(widths[2], layers[2], stride=(1, 2))
        self.layer4 = self._make_layer(widths[3], layers[3], stride=(2, 2))
        self.avgpool = torch.nn.AdaptiveAvgPool2d((1, 1))
        self.fc = torch.nn.Linear(widths[3] * BasicBlock.expansion, num_outputs)
        self.layer4[-1].pad_out = False
        for m in self.modules():                       # resnet_modified.py:64-66
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity=activation_fct)

    def _make_layer(self, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * BasicBlock.expansion:
            downsample = torch.nn.Sequential(
                torch.nn.Conv2d(self.inplanes, planes * BasicBlock.expansion, kernel_size=1, stride=stride, bias=False))
        stack = [BasicBlock(self.inplanes, planes, stride=stride, downsample=downsample, activation_fct=self.activation_fct)]
        self.inplanes = planes * BasicBlock.expansion
        stack += [BasicBlock(self.inplanes, planes, activation_fct=self.activation_fct) for _ in range(1, blocks)]
        return torch.nn.Sequential(*stack)

    def _trunk_blocks(self):
        blocks, weights = [], []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                stride = blk.stride if isinstance(blk.stride, tuple) else (blk.stride, blk.stride)
                has_ds = blk.downsample is not None
                blocks.append((blk.conv1.in_channels, blk.conv1.out_channels, tuple(stride), has_ds))
                weights += [blk.conv1.weight, blk.conv2.weight] + ([blk.downsample[0].weight] if has_ds else [])
        return tuple(blocks), weights

    def trunk_weights_channels_last(self):
        """Store the trunk's convolution weights as ``[K][k][k][C]`` (torch channels_last): the HIP trunk then reads the
        parameters and writes their gradients in place.  Shapes, names and values of the state_dict do not change; conv1
        (8 input channels, re-laid out per call: 4.6 kB) keeps the default layout."""
        for w in self._trunk_blocks()[1]:
            w.data = w.data.contiguous(memory_format=torch.channels_last)
        return self

    def _note_module_path(self, x, why=None):
        """One line per (shape, dtype, mode) whenever a CUDA input takes the module path (library convolutions + ring ops) instead of
        the HIP stem + trunk: a 5x slower path must not be taken silently (factor-8 networks, widths not divisible by 4).
        ``why``: the caller's own reason (the feature tower in front of this network, models/model.py)."""
        if not x.is_cuda or self.impl == "modules":
            return
        key = (tuple(x.shape), x.dtype, torch.is_autocast_enabled(), self.training and self.use_dropout)
        seen = self.__dict__.setdefault("_module_path_noted", set())
        if key not in seen:
            seen.add(key)
            why = why or ("autocast shapes do not tile (csrc/convh.hip)" if key[2]
                          else "channel counts are neither multiples of 64 nor a narrow network's 16 / 32 (factor_fewer_resnet_channels 2 and 4 "
                          "of an 8-channel input), or the width is not a multiple of 4"
                          + (" (with dropout the HIP stem has to take the input as well as the trunk)" if key[3] else ""))
            print(f"[delora_amd] CNN input {key[0]} {str(x.dtype).replace('torch.', '')} runs on the MODULE path (library convolutions), "
                  f"not on the HIP stem + trunk: {why}", flush=True)

    def hip_path_takes(self, H, W, in_channels=None, batch=1):
        """Whether an ``[N,in_channels,H,W]`` fp32 CUDA input (default: this network's own input channels -- 8, or the feature
        tower's 80) would run on the channels-last HIP stem + trunk (shape test only: ``ring_conv.supported`` / ``stem_supported``:
        full-width channel counts or those of factor_fewer_resnet_channels 2 and 4 on the 8-channel input, a width divisible by 4).  True for BASELINE's
        images and for the reference's shipped 64 x 720 and 64 x 512 (tiles hang over the edges of maps that do not divide)."""
        if self.impl == "modules" or W % 4:
            return False
        C0 = self.conv1.out_channels
        if in_channels is None:
            in_channels = self.conv1.in_channels
        if in_channels == ring_conv.TOWER_CHANNELS and not ring_conv.tower_supported((batch, 8, H, W)):
            return False
        return (ring_conv.stem_supported((batch, in_channels, H, W), C0)
                and ring_conv.supported((batch, H, W // 4, C0), self._trunk_blocks()[0], narrow=in_channels == 8))

    def hip_trunk_applicable(self, x_pooled_shape_nhwc, x, narrow=True):
        """The HIP trunk runs fp32 CUDA tensors outside autocast on shapes that tile (with or without dropout): channel counts multiples
        of 64, or -- ``narrow`` -- a narrow network's (``ring_conv.supported``)."""
        if self.impl == "modules" or not x.is_cuda or x.dtype != torch.float32 or torch.is_autocast_enabled():
            return False
        return ring_conv.supported(x_pooled_shape_nhwc, self._trunk_blocks()[0], narrow=narrow)

    def hip_half_applicable(self, x):
        """The half-precision HIP trunk (``ring_conv.RingTrunkH``) runs CUDA inputs inside ``torch.autocast`` (fp16 / bf16) on shapes
        that tile (with or without dropout); returns the autocast dtype or None."""
        if self.impl == "modules" or not x.is_cuda or not torch.is_autocast_enabled():
            return None
        dtype = torch.get_autocast_dtype("cuda")
        N, Cin, Hin, Win = x.shape
        C0 = self.conv1.out_channels
        if dtype not in ring_conv.DTYPE_CODE or Win % 4 or not ring_conv.planar_stem_supported((N, Cin, Hin, Win), C0):
            return None
        return dtype if ring_conv.supported_h((N, Hin, Win // 4, C0), self._trunk_blocks()[0]) else None

    def hip_half_stem_applicable(self, x):
        """Whether the stem too runs in half precision (``ring_conv.RingStemH``): ``amp_stem`` is set, the half-precision trunk takes the
        input (``hip_half_applicable``), conv1 is the 8 -> 64 layer, dropout is not active (its input mask lives in the fp32 copy) and
        the image needs no gradient (the half stem computes none).  Returns the autocast dtype or None."""
        if not self.amp_stem or self.dropout_active() or x.requires_grad:
            return None
        if self.conv1.in_channels != 8 or self.conv1.out_channels != 64:
            return None
        half = self.hip_half_applicable(x)
        if half is None or x.dtype != torch.float32 or not ring_conv.stem_h_supported(tuple(x.shape), self.conv1.out_channels):
            return None
        return half

    def dropout_active(self):
        return self.use_dropout and self.training

    def _draw_dropout(self, x, c3):
        """Seed and the two small masks of one forward pass (kept in ``last_dropout`` for inspection; under a captured graph these are
        the static tensors every replay overwrites): (stem argument, trunk argument, fc scale)."""
        N = x.shape[0]
        rank, world = 0, 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        seed = ring_conv.mix_rank(ring_conv.draw_seed(x.device), rank, world)
        p = float(self.dropout_p)
        channels = ring_conv.dropout_scale(seed, ring_conv.SITE_CHANNELS, p, N * c3).view(N, c3)
        fc = ring_conv.dropout_scale(seed, ring_conv.SITE_FC, p, N * self.fc.out_features).view(N, self.fc.out_features)
        self.last_dropout = {"seed": seed, "p": p, "channels": channels, "fc": fc}
        return (seed, p), (channels, len(self.layer1) + len(self.layer2) + len(self.layer3)), fc

    def pooled_features(self, x):
        """The globally pooled feature ``[N,C']`` (fp32; the input of ``fc``) when the whole CNN runs on the HIP stem + trunk -- fp32, or
        half precision inside autocast -- else None.  Returns (feat, last feature map as NCHW view or None)."""
        return self.pooled_features_drop(x)[:2]

    def pooled_features_drop(self, x):
        """``pooled_features`` plus the third element the heads need when dropout is active: the scale ``[N,R]`` (0 or 1 / (1 - p)) to
        apply to the fc output, else None.  With active dropout one seed is drawn per call -- only once the HIP path is known to take
        the input -- and serves the three sites."""
        act = "relu" if self.activation_fct == "relu" else "tanh"
        N, Cin, Hin, Win = x.shape
        C0 = self.conv1.out_channels
        half = self.hip_half_applicable(x)
        if half is not None:
            # autocast: fp32 stem (8 input channels: 0.4 ms), then layer1..layer4 + pooling on the half-precision MFMA kernels
            blocks, weights = self._trunk_blocks()
            if self.hip_half_stem_applicable(x) is not None:
                # amp_stem: conv1, the pooling and the fused weight gradient in the autocast dtype as well; no fp32 map, no cast launch
                with torch.autocast("cuda", enabled=False):
                    x0 = ring_conv.RingStemH.apply(x, self.conv1.weight, ring_conv.ACT[act], half)          # [N,H,W/4,C0] half
                    feat = ring_conv.ring_trunk_h(x0, ring_conv.ACT[act], blocks, half, weights, x0_is_half=True)
                return feat, None, None
            with torch.autocast("cuda", enabled=False):
                d_ch = fc_scale = None
                if self.dropout_active():
                    d_in, d_ch, fc_scale = self._draw_dropout(x, self.layer3[-1].conv2.out_channels)
                    x0 = ring_conv.RingStem.apply(x.float(), self.conv1.weight, ring_conv.ACT[act], d_in)
                else:
                    x0 = ring_conv.RingStem.apply(x.float(), self.conv1.weight, ring_conv.ACT[act])      # [N,H,W/4,C0] fp32
                feat = ring_conv.ring_trunk_h(x0, ring_conv.ACT[act], blocks, half, weights, channel_drop=d_ch)      # [N,C'] fp32
            return feat, None, fc_scale
        if (self.hip_trunk_applicable((N, Hin, Win // 4, C0), x) and Win % 4 == 0
                and ring_conv.planar_stem_supported(tuple(x.shape), C0)):
            # channels-last from the first layer on: stem (conv1 + act + pool) and layer1..layer4 on the HIP kernels
            blocks, weights = self._trunk_blocks()
            d_ch = fc_scale = None
            if self.dropout_active():
                d_in, d_ch, fc_scale = self._draw_dropout(x, self.layer3[-1].conv2.out_channels)
                x0 = ring_conv.RingStem.apply(x, self.conv1.weight, ring_conv.ACT[act], d_in)
            else:
                x0 = ring_conv.RingStem.apply(x, self.conv1.weight, ring_conv.ACT[act])          # [N,H,W/4,C0]
            x4 = ring_conv.ring_trunk(x0, ring_conv.ACT[act], blocks, weights, channel_drop=d_ch)       # [N,H',W',C']
            return ring_conv.MeanHW.apply(x4), x4.permute(0, 3, 1, 2), fc_scale
        return None, None, None

    def wide_path_dtype(self, stacked, pair=False):
        """Whether the planar image pair ``[B,8,H,W]`` of a network behind the feature tower runs on the HIP tower + wide stem + trunk:
        an fp32 CUDA tensor, a full-width network with 80 input channels, a width divisible by 4 (with or without dropout).  Returns None
        (no), torch.float32, or -- inside ``torch.autocast`` -- the half-precision dtype the trunk then runs in.  ``pair``: ``stacked``
        is the first ``[B,4,H,W]`` image of a pair that has not been concatenated yet (a shape test before the copy)."""
        if (self.impl == "modules" or not stacked.is_cuda or stacked.dtype != torch.float32
                or self.conv1.in_channels != ring_conv.TOWER_CHANNELS or stacked.dim() != 4):
            return None
        B, C, H, W = stacked.shape
        if pair:
            C *= 2
        C0 = self.conv1.out_channels
        if W % 4 or not ring_conv.tower_supported((B, C, H, W)) or not ring_conv.stem_supported((B, ring_conv.TOWER_CHANNELS, H, W), C0):
            return None
        blocks = self._trunk_blocks()[0]
        if torch.is_autocast_enabled():
            dtype = torch.get_autocast_dtype("cuda")
            return dtype if dtype in ring_conv.DTYPE_CODE and ring_conv.supported_h((B, H, W // 4, C0), blocks) else None
        return torch.float32 if ring_conv.supported((B, H, W // 4, C0), blocks) else None

    def pooled_features_wide(self, stacked, tower_weights, dtype):
        """The globally pooled feature ``[B,C']`` (fp32) of an image pair behind the feature tower, all on HIP kernels: ``RingTower``
        and ``RingStemWide`` in fp32 (inside autocast too, as the 8-channel stem), then the trunk in ``dtype`` (``wide_path_dtype``).
        Returns (feat, last feature map as NCHW view or None, fc scale or None).  With active dropout one seed is drawn per call and
        serves the three sites: the element-wise mask on the 80 tower channels inside ``RingTowerDrop``, the channel mask behind
        layer3 in the trunk, and the scale ``[B,R]`` for the fc output that goes back to the caller (as ``pooled_features_drop``)."""
        act = ring_conv.ACT["relu" if self.activation_fct == "relu" else "tanh"]
        blocks, weights = self._trunk_blocks()
        with torch.autocast("cuda", enabled=False):
            d_ch = fc_scale = None
            if self.dropout_active():
                (seed, p), d_ch, fc_scale = self._draw_dropout(stacked, self.layer3[-1].conv2.out_channels)
                xw = ring_conv.RingTowerDrop.apply(stacked, act, seed, p, *tower_weights)   # [B,H,W,128]: dropped, channels 80.. zero
                x0 = ring_conv.RingStemWide.apply(xw, self.conv1.weight, act, False)        # (False: the true dL/dxw goes back)
            else:
                xw = ring_conv.RingTower.apply(stacked, act, False, *tower_weights)        # [B,H,W,128], channels 80.. zero
                x0 = ring_conv.RingStemWide.apply(xw, self.conv1.weight, act, True)         # [B,H,W/4,C0]
            if dtype != torch.float32:
                return ring_conv.ring_trunk_h(x0, act, blocks, dtype, weights, channel_drop=d_ch), None, fc_scale
            x4 = ring_conv.ring_trunk(x0, act, blocks, weights, channel_drop=d_ch)
            return ring_conv.MeanHW.apply(x4), x4.permute(0, 3, 1, 2), fc_scale

    def forward(self, x):
        act = "relu" if self.activation_fct == "relu" else "tanh"
        N, Cin, Hin, Win = x.shape
        C0 = self.conv1.out_channels
        feat, x4, fc_scale = self.pooled_features_drop(x)          # (the HIP path applies the input and channel dropout itself)
        if feat is not None:
            with torch.autocast("cuda", enabled=False):
                out = self.fc(feat)
                if fc_scale is not None:
                    out = out * fc_scale                            # the same mask the fused heads would apply
            return [None, None, None, x4, out]
        x = self.dropout_values(x)
        p = ring_act_pad(x, "none", pad=True)
        p = ring_act_pool_pad(self.conv1(p), act)                    # act + wrap + self.maxpool + wrap, fused
        N, C0, H0, Wp = p.shape
        # (a narrow network gets here only with an input the HIP stem refuses -- the feature tower's 80 channels, a width that is not a
        # multiple of 4: it stays on the module path as a whole)
        if not self.dropout_active() and self.hip_trunk_applicable((N, H0, Wp - 2, C0), p, narrow=False):
            # channels-last trunk: layer1..layer4 as one autograd Function on the fp32 matrix cores
            blocks, weights = self._trunk_blocks()
            if Cin == ring_conv.TOWER_CHANNELS:        # behind the feature tower: tower and stem ran as library convolutions
                self._note_module_path(x, why="the feature tower and the stem run as library convolutions (a width that is not a multiple "
                                       "of 4, or an input the HIP tower does not take); layer1..layer4 run on the HIP trunk")
            x0 = p[..., 1:-1].permute(0, 2, 3, 1).contiguous()
            x4 = ring_conv.RingTrunk.apply(x0, ring_conv.ACT[act], blocks, *weights)          # [N,H',W',C']
            out = self.fc(ring_conv.MeanHW.apply(x4))
            return [None, None, None, x4.permute(0, 3, 1, 2), out]
        if self.impl == "hip":
            raise RuntimeError(f"cnn_impl 'hip': the HIP trunk does not support input {tuple(x.shape)} / dtype {x.dtype}")
        self._note_module_path(x)
        p1 = self.layer1(p)
        p2 = self.layer2(p1)
        p3 = self.dropout_channels(self.layer3(p2))
        x4 = self.layer4(p3)                                         # unpadded (last block)
        out = self.dropout_values(self.fc(torch.flatten(self.avgpool(x4), 1)))
        # the reference returns the four feature maps as well; they are views of the padded tensors here
        return [p1[..., 1:-1], p2[..., 1:-1], p3[..., 1:-1], x4, out]
