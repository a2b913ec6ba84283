"""Generate tests/golden/train_bn_parts.npz: inputs, outputs and autograd gradients of the reference's CNNBlock
(model.py:5-18: Conv2d 3x3 pad 1, BatchNorm2d, LeakyReLU(0.1)) in train() mode -- batch statistics -- for (Ci, Co, H, W, B)
= (3, 8, 5, 5, 3), in f64, and BatchNorm's three buffers after one and after two forwards. Runs only where the read-only
reference checkout is present (tests/golden/_ref_import.py); only the data it writes is committed.

    python tests/golden/make_golden_train_bn.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import import_reference  # noqa: E402

CI, CO, H, W, B = 3, 8, 5, 5, 3


def main():
    import_reference()
    from reference.axtrack.machinelearning.model import CNNBlock
    rng = np.random.default_rng(20261020)
    block = CNNBlock(CI, CO, nn.LeakyReLU(0.1), kernel_size=3, padding=1).double()
    tensors = {
        'conv.weight': rng.uniform(-1, 1, (CO, CI, 3, 3)) / np.sqrt(9 * CI),
        'conv.bias': rng.uniform(-1, 1, CO) / np.sqrt(9 * CI),
        'batchnorm.weight': rng.uniform(0.5, 1.5, CO) * np.where(np.arange(CO) % 3 == 1, -1.0, 1.0),
        'batchnorm.bias': rng.normal(0, 0.2, CO),
        'batchnorm.running_mean': rng.normal(0, 0.2, CO),
        'batchnorm.running_var': rng.uniform(0.5, 1.5, CO),
    }
    # f32-representable values, so that the test can hand the same numbers to an f32 implementation
    tensors = {k: v.astype(np.float32).astype(np.float64) for k, v in tensors.items()}
    block.load_state_dict({**{k: torch.from_numpy(v) for k, v in tensors.items()},
                           'batchnorm.num_batches_tracked': torch.tensor(7)})
    block.train()
    x = torch.from_numpy(rng.normal(0, 1, (B, CI, H, W)).astype(np.float32).astype(np.float64)).requires_grad_(True)
    x2 = torch.from_numpy(rng.normal(0, 1, (B, CI, H, W)).astype(np.float32).astype(np.float64))
    dF = torch.from_numpy(rng.normal(0, 1, (B, CO, H, W)).astype(np.float32).astype(np.float64))
    out = block(x)
    out.backward(dF)
    bn = block.batchnorm
    res = {k.replace('.', '_'): v for k, v in tensors.items()}
    res.update(x=x.detach().numpy(), x2=x2.numpy(), dF=dF.numpy(), F=out.detach().numpy(), grad_x=x.grad.numpy(),
               grad_conv_weight=block.conv.weight.grad.numpy(), grad_conv_bias=block.conv.bias.grad.numpy(),
               grad_batchnorm_weight=bn.weight.grad.numpy(), grad_batchnorm_bias=bn.bias.grad.numpy(),
               momentum=np.float64(bn.momentum), eps=np.float64(bn.eps),
               running_mean_1=bn.running_mean.numpy().copy(), running_var_1=bn.running_var.numpy().copy(),
               num_batches_tracked_1=np.int64(int(bn.num_batches_tracked)))
    with torch.no_grad():
        block(x2)
    res.update(running_mean_2=bn.running_mean.numpy().copy(), running_var_2=bn.running_var.numpy().copy(),
               num_batches_tracked_2=np.int64(int(bn.num_batches_tracked)))
    assert res['num_batches_tracked_1'] == 8 and res['num_batches_tracked_2'] == 9
    np.savez_compressed(os.path.join(HERE, 'train_bn_parts.npz'), **res)
    print({k: v.shape for k, v in res.items()})


if __name__ == '__main__':
    main()
