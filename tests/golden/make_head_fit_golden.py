"""Writes tests/golden/head_fit.npz: the reference's train iteration for a Linear head, recorded for tests/test_head_fit_cpu.py and
tests/test_gpu_head_fit.py.

    python tests/golden/make_head_fit_golden.py /path/to/reference

The reference's src/audio/loss/loss.py (SoftFocalLoss, SoftFocalLossWrapper) is imported from the given tree; the iteration is
tests/head_fit_cases.torch_fit -- NetTrainer.iterate_model's train branch with mixup_data, torch.optim.Adam and
CosineAnnealingWarmRestarts.step(epoch + idx / iters) -- on a torch.nn.Linear in float64.  Per case and run the file holds
w_hist, b_hist, batch_loss, epoch_loss (float64) and f32_dev: the largest absolute deviation of the same iteration in float32
from the float64 one over w_hist, b_hist and batch_loss."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import head_fit_cases as cases  # noqa: E402


def main(reference: str) -> None:
    sys.path.insert(0, os.path.join(reference, "src", "audio"))
    from loss.loss import SoftFocalLoss, SoftFocalLossWrapper

    def focal(alpha, gamma):
        return SoftFocalLossWrapper(SoftFocalLoss(alpha=alpha, gamma=gamma), num_classes=classes)

    out = {}
    for name in cases.GOLDEN:
        feats, targets, runs, bsz = cases.inputs(name)
        classes = cases.shape(name)[1]
        for r, run in runs.items():
            want = cases.torch_fit(feats, targets, run, bsz, torch.float64, focal=focal)
            low = cases.torch_fit(feats, targets, run, bsz, torch.float32, focal=focal)
            for key, value in zip(want._fields, want):
                out[f"{name}/{r}/{key}"] = value
            out[f"{name}/{r}/f32_dev"] = np.float64(cases.deviation(low, want))
            print(f"{name:10s} {r:10s} f32_dev {out[f'{name}/{r}/f32_dev']:.3e}  epoch_loss {want.epoch_loss}")
    np.savez(os.path.join(HERE, "head_fit.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
