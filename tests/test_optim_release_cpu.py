"""A dropped FlatParams / FlatAdamWEMA pair gives its buffers back at once, by reference counting: the optimiser holds its FlatParams, the FlatParams
reaches the optimiser (for `begin_step`'s wait on an overlapped step) only weakly.  With a strong back-reference the pair is a cycle, and the flat weights,
gradients, EMA and both moment buffers of a dropped trainer stay allocated until the cyclic collector's next full pass -- gigabytes on the device, at a moment
nobody controls."""
import gc
import weakref

import torch


def test_dropped_flat_optimiser_frees_its_buffers_without_the_cyclic_collector():
    from dmvae_amd.optim import FlatAdamWEMA, FlatParams
    params = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    gc.collect()
    gc.disable()
    try:
        fp = FlatParams(params, with_ema=True)
        opt = FlatAdamWEMA(fp, lr=1e-3, warmup_steps=0)
        assert fp._opt() is opt                                   # begin_step still finds the optimiser it has to wait for
        fp.begin_step()
        refs = [weakref.ref(t) for t in (fp.flat, fp.grad, fp.ema, opt.exp_avg, opt.exp_avg_sq)] + [weakref.ref(fp), weakref.ref(opt)]
        for p in params:                                          # the parameters outlive the trainer in a caller's module: they hold views, not the pair
            p.data, p.grad = torch.zeros(0), None
            p.__dict__.clear()
        del fp, opt, p
        assert [r() is None for r in refs] == [True] * len(refs)
    finally:
        gc.enable()


def test_flat_params_without_an_optimiser_begins_a_step():
    from dmvae_amd.optim import FlatParams
    fp = FlatParams([torch.nn.Parameter(torch.randn(4))], with_ema=False)
    fp.begin_step()
    assert fp.grad.abs().sum() == 0
