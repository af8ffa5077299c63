"""The dynamic-LDS opt-in (csrc/common.h DMVAE_LDS_OPTIN -> api.hip::dmvae_lds_optin) is kept per (launch site, device): a kernel that needs more than the default
64 KB of LDS must launch on the SECOND device a process uses as it does on the first.  A process-wide "already set" flag would leave device 1 without the
attribute and its launch refused.

The launch exercised: `ops.linear_bf16` -> dmvae_linear_bf16 -> gemm_pp.hip::dispatch<false> -> dmvae_gemm_pp::launch<TM, TP, WM, WP, false> of the menu tile that
`ops.linear_plan` names.  That launcher's ring needs nbuf * (TM + TP) * 64 + 3 KiB of LDS, more than 64 KB for every tile of the menu (checked below for the
tile in use).  Shape: M = N = 256 at K = 384, the kernel's minimum reduction -- one or two tiles, microseconds.

Needs two visible devices; on a one-GPU machine it skips and the per-device claim rests on reading dmvae_lds_optin."""
import pytest
import torch

pytestmark = pytest.mark.gpu
M, N, K = 256, 256, 384


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs in one process")
def test_large_lds_kernel_launches_on_a_second_device_of_the_process():
    from dmvae_amd import ops

    _, tc, tr = ops.linear_plan(M, N, K)
    slot = (tc + tr) * 64
    lds = min(6, (160 * 1024 - 3 * 1024) // slot) * slot + 3 * 1024     # gemm_pp.hip::launch
    assert lds > 64 * 1024, (tc, tr, lds)

    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    out = []
    for d in (0, 1):
        with torch.cuda.device(d):
            y = ops.linear_bf16(x.to(f"cuda:{d}"), w.to(f"cuda:{d}"))     # raises DmvaeHipError if the launch is refused
            torch.cuda.synchronize()
            assert y.device.index == d
            out.append(y.cpu())
    assert out[0].abs().max().item() > 0
    assert torch.equal(out[0].view(torch.int16), out[1].view(torch.int16))
