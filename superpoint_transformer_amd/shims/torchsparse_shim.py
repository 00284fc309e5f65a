"""``torchsparse`` (CUDA-only): the names src/nn/sparse.py and src/nn/stage.py import -
``torchsparse.SparseTensor`` and ``torchsparse.nn.{Conv3d, ReLU, LeakyReLU, SiLU}`` - bound to
``superpoint_transformer_amd.nn.sparse``, so the reference's own ``SparseCNN`` constructs and
runs on the HIP sparse convolution.  Stride-1, odd kernel sizes only."""
import types

from ..nn.sparse import Conv3d, LeakyReLU, ReLU, SiLU, SparseTensor

__all__ = ["SparseTensor", "nn"]

nn = types.ModuleType("torchsparse.nn")
nn.Conv3d, nn.ReLU, nn.LeakyReLU, nn.SiLU = Conv3d, ReLU, LeakyReLU, SiLU
