"""_lib.call with tensors on the device: the same launch as with raw pointers, and a refused
tensor leaves its memory alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def test_argmax_with_tensors_equals_argmax_with_pointers():
    import pcs_amd._lib as L
    g = torch.Generator().manual_seed(3)
    z = torch.randn(5, 3, generator=g).to(DEV)
    by_tensor = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    by_ptr = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    s = L.stream_ptr()
    L.call("pcs_argmax", z, z.stride(0), 5, 3, by_tensor, s)
    L.call("pcs_argmax", L.ptr(z), z.stride(0), 5, 3, L.ptr(by_ptr), s)
    assert torch.equal(by_tensor, by_ptr) and torch.equal(by_tensor.cpu(), torch.argmax(z.cpu(), 1))
    out32 = torch.full((5,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError, match=r"pcs_argmax: out is int64_t \*, got a torch\.int32 tensor"):
        L.call("pcs_argmax", z, z.stride(0), 5, 3, out32, s)
    torch.cuda.synchronize()
    assert torch.equal(out32.cpu(), torch.full((5,), -7, dtype=torch.int32))
