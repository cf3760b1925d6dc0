"""Pose regression network: stacked range-image pair -> (translation[B,3], quaternion[B,4] as x,y,z,w).
Mirror of the reference's OdometryModel (src/models/model.py:16-116) with identical parameter names."""
import torch

from . import model_parts, resnet_modified


def _act(name):
    return torch.nn.ReLU() if name == "relu" else torch.nn.Tanh()


def _mlp(name, sizes):
    layers = []
    for fan_in, fan_out in zip(sizes[:-1], sizes[1:]):
        layers += [_act(name), torch.nn.Linear(fan_in, fan_out)]
    return torch.nn.Sequential(*layers)


class OdometryModel(torch.nn.Module):
    def __init__(self, config):
        super().__init__()
        self.device = config["device"]
        self.config = config
        act = config["activation_fct"]
        if act not in ("relu", "tanh"):
            raise Exception('The specified activation function must be either "relu" or "tanh".')
        self.pre_feature_extraction = config["pre_feature_extraction"]
        in_channels, n_pre = 8, 5
        if self.pre_feature_extraction:                  # model.py:31-48: per-image conv tower before stacking
            tower = []
            for i in range(n_pre):
                c_in = in_channels // 2 if i == 0 else i * in_channels
                tower += [model_parts.CircularPad(padding=(1, 1, 0, 0)),
                          torch.nn.Conv2d(c_in, (i + 1) * in_channels, kernel_size=3, padding=(1, 0), bias=False),
                          torch.nn.ReLU(inplace=True) if act == "relu" else torch.nn.Tanh()]
            self.feature_extractor = torch.nn.Sequential(*tower)
        self.resnet = resnet_modified.ResNetModified(
            in_channels=in_channels if not self.pre_feature_extraction else 2 * n_pre * in_channels,
            num_outputs=config["resnet_outputs"], use_dropout=config["use_dropout"], layers=config["layers"],
            factor_fewer_resnet_channels=config["factor_fewer_resnet_channels"], activation_fct=act,
            impl=config.get("cnn_impl", "auto"))
        self.resnet.amp_stem = bool(config.get("amp_stem", False))       # the stem in the autocast dtype too (default: fp32)
        n_feat = config["resnet_outputs"]
        if config["use_single_mlp_at_output"]:           # model.py:59-72
            self.fully_connected_rot_trans = _mlp(act, [n_feat, 512, 512, 256, 64, 3 + 4])
        else:                                            # model.py:74-83
            self.fully_connected_rotation = _mlp(act, [n_feat, 100, 4])
            self.fully_connected_translation = _mlp(act, [n_feat, 100, 3])
        self.geometry_handler = model_parts.GeometryHandler(config=config)

    def _tower_weights(self):
        return [m.weight for m in self.feature_extractor if isinstance(m, torch.nn.Conv2d)]

    def _fused(self, pooled, fc_scale):
        """fc + heads as ONE autograd Function on the pooled feature: ``FusedHeads`` for the two heads, ``FusedHeadsSingle`` for
        ``use_single_mlp_at_output``; ``fc_scale`` (the dropout mask of the fc output, or None) travels into either as a factor."""
        act = 2 if self.config["activation_fct"] == "relu" else 1
        extra = [fc_scale] if fc_scale is not None else []
        with torch.autocast("cuda", enabled=False):
            if self.config["use_single_mlp_at_output"]:
                linears = [m for m in self.fully_connected_rot_trans if isinstance(m, torch.nn.Linear)]
                params = [self.resnet.fc.weight, self.resnet.fc.bias] + [t for m in linears for t in (m.weight, m.bias)]
                return model_parts.FusedHeadsSingle.apply(pooled.float(), act, *params, *extra)
            fr, ft = self.fully_connected_rotation, self.fully_connected_translation
            return model_parts.FusedHeads.apply(pooled.float(), act, self.resnet.fc.weight, self.resnet.fc.bias, fr[1].weight, fr[1].bias,
                                                fr[3].weight, fr[3].bias, ft[1].weight, ft[1].bias, ft[3].weight, ft[3].bias, *extra)

    def forward_tower(self, stacked):
        """``pre_feature_extraction`` on the HIP path: the planar pair ``[B,8,H,W]`` through ``ring_conv.RingTower`` (five narrow MFMA
        layers per image, both images per launch; ``RingTowerDrop`` with active dropout), ``RingStemWide``, the trunk and the fused
        heads.  Returns None when that path does not take the input (``ResNetModified.wide_path_dtype``: CPU tensors, narrow networks,
        widths not divisible by 4, ``cnn_impl: modules``); ``cnn_impl: hip`` makes that an error."""
        dtype = self.resnet.wide_path_dtype(stacked)
        if dtype is None:
            if self.config.get("cnn_impl", "auto") == "hip" and stacked.is_cuda:
                raise RuntimeError(f"cnn_impl 'hip': the HIP feature tower does not support input {tuple(stacked.shape)} / dtype {stacked.dtype} "
                                   "(it takes fp32 pairs of a full-width network whose width is a multiple of 4)")
            return None                      # (the resnet prints the one module-path note for its 80-channel input)
        pooled, _, fc_scale = self.resnet.pooled_features_wide(stacked, self._tower_weights(), dtype)
        if self._fused_heads_ok(stacked):
            return self._fused(pooled, fc_scale)
        with torch.autocast("cuda", enabled=False):
            out = self.resnet.fc(pooled)
            if fc_scale is not None:
                out = out * fc_scale                                # the same mask the fused heads would apply
            return self._heads(out)

    def forward_features(self, image_1, image_2):
        if self.pre_feature_extraction:
            x = torch.cat((self.feature_extractor(image_1), self.feature_extractor(image_2)), dim=1)
        else:
            x = torch.cat((image_1, image_2), dim=1)
        return self.resnet(x)

    def forward_stacked(self, stacked):
        """Same as forward() for an already channel-stacked ``[B,8,H,W]`` pair (no concatenation copy).  When the CNN runs on the HIP
        stem + trunk, fc and the heads run as ``model_parts.FusedHeads`` (csrc/heads.hip: 3 + 4 launches instead of ~45) or, for
        ``use_single_mlp_at_output``, as ``model_parts.FusedHeadsSingle`` (6 + 11 instead of ~65); with active dropout the fc output's
        mask travels into them as a factor."""
        if self._fused_heads_ok(stacked):
            pooled, _, fc_scale = self.resnet.pooled_features_drop(stacked)
            if pooled is not None:
                return self._fused(pooled, fc_scale)
        feat = self.resnet(stacked)[-1]
        return self._heads(feat)

    def _fused_heads_ok(self, x):
        """fc + heads as one fused Function (either head architecture): CUDA input, a batch of at most 16 (dropout on the fc output
        is a factor inside the fused kernels: ``dl_heads_fwd_drop``, the ``fc_scale`` of ``dl_heads_single_fwd``)."""
        return (x.is_cuda and x.shape[0] <= 16 and self.config.get("fused_heads", True)
                and self.config.get("cnn_impl", "auto") != "modules")

    def _heads(self, feat):
        if self.config["use_single_mlp_at_output"]:
            y = self.fully_connected_rot_trans(feat)
            rotation, translation = y[:, :4], y[:, 4:]
        else:
            rotation = self.fully_connected_rotation(feat)
            translation = self.fully_connected_translation(feat)
        # model.py:114: one norm over the WHOLE batch of quaternions (the per-row normalisation happens later,
        # inside quaternion -> R); kept because it is part of the gradient path
        rotation = rotation / torch.norm(rotation)
        return translation, rotation

    def forward(self, image_1, image_2=None):
        """``forward(image_1, image_2)`` as the reference; ``forward(stacked)`` with a ``[B,8,H,W]`` tensor skips the
        concatenation copy.  With the per-image feature tower both forms take ``forward_tower`` when the HIP path takes the input
        (the gate is decided on the shapes before anything is copied), else the tower's modules on the two images."""
        if image_2 is None:
            if self.pre_feature_extraction:
                out = self.forward_tower(image_1)
                if out is not None:
                    return out
                image_1, image_2 = image_1[:, :4], image_1[:, 4:]
            else:
                return self.forward_stacked(image_1)
        elif self.pre_feature_extraction and (self.resnet.wide_path_dtype(image_1, pair=True) is not None
                                              or (image_1.is_cuda and self.config.get("cnn_impl", "auto") == "hip")):
            out = self.forward_tower(torch.cat((image_1, image_2), dim=1))          # (two 4-channel images: the only copy)
            if out is not None:
                return out
        return self._heads(self.forward_features(image_1=image_1, image_2=image_2)[-1])
