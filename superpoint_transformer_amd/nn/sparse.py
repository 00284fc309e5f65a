"""Sparse CNN point encoder (src/nn/sparse.py) on ``superpoint_transformer_amd.sparse``.

``SparseTensor`` / ``Conv3d`` / ``ReLU`` / ``LeakyReLU`` / ``SiLU`` stand in for the torchsparse
classes of the same names (``shims/torchsparse_shim.py`` exports them under those import names);
``ConvBlock`` and ``SparseCNN`` keep the reference's constructor arguments, module names and
state-dict keys (``N.conv.kernel``, ``N.norm.*``).  One kernel map is built per distinct
``(kernel_size, dilation)`` and per forward: the map cache travels with the ``SparseTensor``
from block to block (a stride-1 convolution keeps the coordinates)."""
import logging

import torch
from torch import nn

from .. import sparse as S
from .norm import GraphNorm, INDEX_BASED_NORMS

log = logging.getLogger(__name__)

__all__ = ["SparseTensor", "Conv3d", "ReLU", "LeakyReLU", "SiLU", "ConvBlock", "SparseCNN"]


class SparseTensor:
    """``coords`` [N, 4] int, batch first then (x, y, z); ``feats`` [N, C].  ``F`` / ``C`` as in
    torchsparse; ``+`` adds the features of two tensors over the same voxels."""

    def __init__(self, feats, coords, stride=1, maps=None):
        if coords.dim() != 2 or coords.shape[1] != 4:
            raise ValueError(f"coords must be [N, 4] (batch, x, y, z), got {tuple(coords.shape)}")
        if feats.shape[0] != coords.shape[0]:
            raise ValueError("feats and coords must hold one row per voxel")
        S.check_stride(stride)
        self.feats, self.coords, self.stride = feats, coords, stride
        self._maps = {} if maps is None else maps           # (kernel_size, dilation) -> KernelMap

    @property
    def F(self):
        return self.feats

    @F.setter
    def F(self, feats):
        self.feats = feats

    @property
    def C(self):
        return self.coords

    @property
    def s(self):
        return self.stride

    def with_feats(self, feats):
        """A tensor over the same voxels (and the same map cache)."""
        return SparseTensor(feats, self.coords, self.stride, self._maps)

    def kernel_map(self, kernel_size, dilation):
        key = (int(kernel_size), int(dilation))
        kmap = self._maps.get(key)
        if kmap is None:
            kmap = self._maps[key] = S.build_kernel_map(self.coords[:, 1:], self.coords[:, 0].long(),
                                                        key[0], key[1])
        return kmap

    def __add__(self, other):
        if not isinstance(other, SparseTensor) or other.coords.shape != self.coords.shape:
            raise ValueError("can only add a SparseTensor over the same voxels")
        return self.with_feats(self.feats + other.feats)

    def to(self, *args, **kwargs):
        return SparseTensor(self.feats.to(*args, **kwargs), self.coords.to(*args, **kwargs),
                            self.stride)


class Conv3d(nn.Module):
    """Stride-1 sparse convolution; parameters ``kernel`` [K^3, C_in, C_out] ([C_in, C_out] for
    K = 1) and ``bias`` [C_out] (optional), initialised as src/utils/nn.py ``_conv_init``."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, bias=False,
                 transposed=False):
        super().__init__()
        S.check_stride(stride, transposed)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = S._kernel_size(kernel_size)
        self.dilation = S._dilation(dilation)
        self.stride, self.transposed = 1, False
        k3 = self.kernel_size ** 3
        shape = (k3, self.in_channels, self.out_channels) if k3 > 1 else \
            (self.in_channels, self.out_channels)
        self.kernel = nn.Parameter(torch.empty(shape))
        if bias:
            self.bias = nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("leaky_relu")
        if self.bias is not None:
            nn.init.constant_(self.bias, 0)
        # fan_in / fan_out are computed on (out, in, volume): a permuted VIEW of the parameter
        view = self.kernel.permute(2, 1, 0) if self.kernel.dim() == 3 else self.kernel.permute(1, 0)
        with torch.no_grad():
            nn.init.xavier_uniform_(view, gain=gain)

    def forward(self, x):
        kmap = x.kernel_map(self.kernel_size, self.dilation)
        return x.with_feats(S.sparse_conv3d(x.feats, self.kernel, kmap, self.bias))

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, "
                f"dilation={self.dilation}, bias={self.bias is not None}")


class _Activation(nn.Module):
    def forward(self, x):
        return x.with_feats(self.fn(x.feats))


class ReLU(_Activation):
    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = inplace

    def fn(self, f):
        return torch.nn.functional.relu(f)


class LeakyReLU(_Activation):
    def __init__(self, negative_slope=0.01, inplace=False):
        super().__init__()
        self.negative_slope, self.inplace = negative_slope, inplace

    def fn(self, f):
        return torch.nn.functional.leaky_relu(f, self.negative_slope)


class SiLU(_Activation):
    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = inplace

    def fn(self, f):
        return torch.nn.functional.silu(f)


class ConvBlock(nn.Module):
    """Conv3d -> norm -> (+ input) -> activation (src/nn/sparse.py:14-83)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, dilation=1, bias=True,
                 norm=None, activation=None, residual=False):
        super().__init__()
        self.conv = Conv3d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                           dilation=dilation, bias=bias)
        if norm is not None and not (isinstance(norm, type) and issubclass(norm, INDEX_BASED_NORMS)):
            raise NotImplementedError(
                f"norm={norm}: only the index-based norms (GraphNorm, LayerNorm, InstanceNorm) run "
                "on a SparseTensor here; torchsparse's own norms are not built")
        self.norm = norm(out_channels) if norm is not None else None
        self.activation = activation
        self.residual = residual
        assert (not self.residual) or in_channels == out_channels, \
            "Residual connection in a block is only supported if the input and output channels " \
            "are the same"

    def forward(self, x, batch=None):
        x_in = x
        x = self.conv(x)
        if self.norm is not None:
            x.F = self.norm(x.F, batch=batch)
        if self.residual:
            x = x + x_in
        if self.activation is not None:
            x = self.activation(x)
        return x


class SparseCNN(nn.ModuleList):
    """src/nn/sparse.py:85-268, same constructor."""

    def __init__(self, cnn, kernel_size, dilation, stride=1, norm=GraphNorm, last_norm=True,
                 activation=ReLU(), last_activation=True, residual=False, global_residual=False,
                 frozen=False):
        super().__init__()
        assert len(cnn) >= 2
        bias = norm is None                                  # a bias only without a normalisation
        self.cnn = cnn
        self.n_blocks = len(cnn) - 1
        self.global_residual = global_residual
        self.frozen = frozen
        assert (not self.global_residual) or cnn[0] == cnn[-1], \
            "Residual connection over the entire CNN is only supported if the input and output " \
            "channels are the same"
        kernel_size = self.check_type(kernel_size)
        stride = self.check_type(stride)
        dilation = self.check_type(dilation)
        residual = self.check_type(residual)
        activation = self._convert_activation(activation)
        if activation is None:
            log.warning("CNN activation function is `None`, no activation will be applied")
        if norm is None:
            log.warning("CNN normalization function is `None`, no normalization will be applied")
        for i, r in enumerate(residual):
            if r:
                assert cnn[i] == cnn[i + 1], \
                    f"Block {i} has residual connection, but the input and output channels are " \
                    f"not the same.\n  Input channels: {cnn[i]}\n  Output channels: {cnn[i + 1]}"
        for i in range(1, len(cnn)):
            last = i == len(cnn) - 1
            self.append(ConvBlock(
                in_channels=cnn[i - 1], out_channels=cnn[i], kernel_size=kernel_size[i - 1],
                stride=stride[i - 1], dilation=dilation[i - 1], bias=bias,
                norm=norm if (last_norm or not last) else None,
                activation=activation if (last_activation or not last) else None,
                residual=residual[i - 1]))

    @property
    def out_dim(self):
        return self.cnn[-1]

    def forward(self, x, batch=None):
        x_in = x
        for block in self:
            x = block(x, batch=batch)
        if self.global_residual:
            x = x + x_in
        return x

    def check_type(self, arg):
        if isinstance(arg, int):                             # (bool is an int: residual)
            return [arg] * self.n_blocks
        if isinstance(arg, (list, tuple)) or type(arg).__name__ == "ListConfig":
            assert len(arg) == self.n_blocks, f"The length of the list must be {self.n_blocks}"
            return arg
        raise ValueError("`kernel_size`, `stride` and `dilation` must be an int or a list of ints")

    def _convert_activation(self, activation):
        if isinstance(activation, (ReLU, LeakyReLU, SiLU)):
            return activation
        if isinstance(activation, nn.Module):
            if isinstance(activation, nn.ReLU):
                return ReLU()
            if isinstance(activation, nn.LeakyReLU):
                return LeakyReLU(negative_slope=activation.negative_slope,
                                 inplace=activation.inplace)
            if isinstance(activation, nn.SiLU):
                return SiLU(inplace=activation.inplace)
            raise ValueError(f"Invalid activation function: {activation}")
        if isinstance(activation, str):
            name = activation.lower()
            if name == "relu":
                return ReLU()
            if name == "leakyrelu":
                return LeakyReLU()
            if name == "silu":
                return SiLU()
            raise ValueError(f"Invalid activation function: {activation}")
        if activation is None:
            return None
        raise ValueError(f"Invalid activation function: {activation}")

    def freeze(self):
        if not self.frozen:
            for param in self.parameters():
                param.requires_grad = False
            self.frozen = True

    def unfreeze(self):
        if self.frozen:
            for param in self.parameters():
                param.requires_grad = True
            self.frozen = False
