"""Shared by the fViT pre-training tests (tests/test_gpu_step_fvit.py, test_fvit_ssl_host.py): the F27 fixture loader
(tools/make_golden_fvit_ssl.py) and the fixture pair's configuration."""
import glob
import os

from conftest import GOLDEN, load_golden

F27_CFG = dict(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, ac_patch_size=12, pad=4, dim=64, depth=2, heads=2,
               mlp_dim=128)
F27_K, F27_B, F27_NLOCAL = 256, 4, 2
BN = "backbone.mlp_head.0."
BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
# the last block's fc2 bias: its gradient is the column sum of the gradient entering the cls rows, i.e. of the BatchNorm input gradient,
# which vanishes identically per group in training mode (tests/test_gpu_fvit.py); ZERO_SUM_SCALE is the same stream's sum one residual
# branch earlier, where nothing cancels
ZERO_SUM, ZERO_SUM_SCALE = "backbone.transformer.layers.1.1.fn.fn.net.3.bias", "backbone.transformer.layers.1.0.fn.fn.to_out.0.bias"


def f27_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "f27_lafs_step_fvit*.npz")))


_F27 = {}


def load_f27():
    """F27 is stored in parts (no committed file above 1 MiB) with disjoint keys; loaded once and shared."""
    if not _F27:
        for path in f27_files():
            part = load_golden(os.path.basename(path)[:-4])
            assert not set(part) & set(_F27), path
            _F27.update(part)
    return _F27
