"""What tests/test_augment_cpu.py and tests/test_gpu_augment.py share: NetTrainer.iterate_model's train iteration in torch, as
tests/head_fit_cases.torch_fit states it, with the rows of every epoch taken from one of several feature tables."""
import numpy as np
import torch

import head_fit_cases as cases


def torch_fit_views(two, targets, run, view, bsz, dtype, epochs):
    """tests/head_fit_cases.torch_fit with the rows of epoch e taken from two[view[e]]"""
    c, f = run.w0.shape
    lin = torch.nn.Linear(f, c).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(run.w0).to(dtype))
        lin.bias.copy_(torch.from_numpy(run.b0).to(dtype))
    weight = None if run.weights is None else torch.from_numpy(np.asarray(run.weights, np.float32)).to(dtype)
    loss = (torch.nn.CrossEntropyLoss(weight=weight, label_smoothing=run.label_smoothing) if run.kind == "ce"
            else cases.soft_focal(weight, run.gamma))
    opt = torch.optim.Adam(lin.parameters(), lr=run.lr, betas=run.betas, eps=run.eps)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=run.t0, eta_min=run.eta_min)
    n = two.shape[1]
    iters = -(-n // bsz)
    y_all = torch.from_numpy(targets)
    w_hist, b_hist, batch_loss = np.zeros((epochs, c, f)), np.zeros((epochs, c)), np.zeros((epochs, iters))
    for e in range(epochs):
        x_all = torch.from_numpy(two[view[e]])
        for idx in range(iters):
            rows = torch.from_numpy(run.order[e, idx * bsz:(idx + 1) * bsz])
            x, y = x_all[rows], y_all[rows]
            if run.mix_lam is not None:
                lam = torch.FloatTensor([run.mix_lam[e, idx]])
                index = torch.from_numpy(run.mix_index[e, idx * bsz:idx * bsz + len(rows)].astype(np.int64))
                hot = torch.nn.functional.one_hot(y, c)
                x = lam * x + (1 - lam) * x[index]
                y = (lam * hot + (1 - lam) * hot[index]).argmax(1)
            opt.zero_grad()
            value = loss(lin(x.to(dtype)).reshape(-1, c), y.flatten())
            value.backward()
            opt.step()
            sched.step(1 + e + idx / iters)
            batch_loss[e, idx] = value.item()
        w_hist[e], b_hist[e] = lin.weight.detach().numpy(), lin.bias.detach().numpy()
    return w_hist, b_hist, batch_loss
