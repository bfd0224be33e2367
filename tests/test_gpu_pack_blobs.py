"""
The four NeRFModel / RefNERFModel weight-packing kernels against blobs built on the host from the index arrays of the
layout library (csrc/nerf_layout.h pack walks, exported by liblnrf_layout_host.so): byte for byte over every region a
kernel writes, no tolerance.  Weights are bf16(params[idx]) with 0 for idx == -1, split streams hold hi = bf16(w) in the even
and lo = bf16(w - float(hi)) in the odd fragments, biases are exact fp32; the region offsets are the library's constants.
The unwritten tail behind a bias block is not compared.
"""
import ctypes

import numpy as np
import pytest
import torch

from learn_nerf import _lib as L
from test_nerf_layout import HOST_LIB, stream_indices

pytestmark = pytest.mark.gpu

N_PARAMS = 593_924  # NeRFModel; RefNERFModel's vector is shorter


@pytest.fixture(scope="module")
def H():
    lib = ctypes.CDLL(HOST_LIB)
    lib.lnrf_host_pack_offset.restype = ctypes.c_int64
    return lib


@pytest.fixture(scope="module")
def params():
    gen = torch.Generator().manual_seed(1234)
    # a wide range of magnitudes, so that the lo halves are not all zero or denormal
    return (torch.randn(N_PARAMS, generator=gen) * torch.exp(2 * torch.randn(N_PARAMS, generator=gen))).float()


def gather(params, idx):
    idx = torch.from_numpy(idx.astype(np.int64))
    return torch.where(idx >= 0, params[idx.clamp(min=0)], torch.zeros(()))


def bf16_bytes(params, idx):
    return gather(params, idx).to(torch.bfloat16).view(torch.uint8)


def split_bytes(params, idx, pairs_of_plain_stream=False):
    """[hi, lo] fragment pairs.  idx is the index array of the split stream itself (both fragments of a pair carry the same
    indices), or, with pairs_of_plain_stream, of a plain stream whose every fragment becomes a pair."""
    w = gather(params, idx).view(-1, 512)
    if pairs_of_plain_stream:
        w = w.repeat_interleave(2, dim=0)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    out = hi.clone()
    out[1::2] = lo[1::2]
    return out.view(torch.uint8).reshape(-1)


def f32_bytes(params, idx):
    return gather(params, idx).view(torch.uint8)


def check_regions(got, regions, blob_bytes):
    assert got.numel() == blob_bytes
    end = 0
    for name, off, want in regions:
        assert off >= end, f"{name} overlaps the region before it"
        end = off + want.numel()
        assert end <= blob_bytes
        have = got[off:end]
        bad = (have != want).nonzero()
        assert bad.numel() == 0, f"{name}: {bad.numel()} bytes differ, first at byte {int(bad[0])} of the region"


def run_pack(fn_name, bytes_fn, params, with_shape):
    lib = L.lib()
    shape = L.NerfShape(5, 4, 256, 128, 10, 4)
    nbytes = bytes_fn(ctypes.byref(shape)) if with_shape else bytes_fn()
    flat = params.cuda()
    packed = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    args = (L.ptr(flat), L.ptr(packed, torch.uint8), L.stream())
    L.check(getattr(lib, fn_name)(*((ctypes.byref(shape),) + args if with_shape else args)), fn_name)
    torch.cuda.synchronize()
    return packed.cpu(), nbytes


def test_nerf_pack_weights(H, params):
    O = H.lnrf_host_pack_offset
    got, n = run_pack("lnrf_nerf_pack_weights", L.lib().lnrf_nerf_packed_bytes, params, True)
    assert n == O(3)
    check_regions(got, [("forward", O(0), bf16_bytes(params, stream_indices(H, "fwd"))),
                        ("transposed", O(1), bf16_bytes(params, stream_indices(H, "bwd"))),
                        ("bias", O(2), f32_bytes(params, stream_indices(H, "bias")))], n)


def test_nerf_pack_weights_split(H, params):
    O = H.lnrf_host_pack_offset
    got, n = run_pack("lnrf_nerf_pack_weights_split", L.lib().lnrf_nerf_packed_split_bytes, params, True)
    assert n == O(5)
    check_regions(got, [("split forward", 0, split_bytes(params, stream_indices(H, "fwd3"))),
                        ("bias", O(4), f32_bytes(params, stream_indices(H, "bias")))], n)


def test_refnerf_trunk_pack(H, params):
    O = H.lnrf_host_pack_offset
    got, n = run_pack("lnrf_refnerf_trunk_pack", L.lib().lnrf_refnerf_trunk_packed_bytes, params, False)
    assert n == O(10)
    check_regions(got, [("forward", O(0), bf16_bytes(params, stream_indices(H, "fwd", ref=True))),
                        ("transposed", O(1), bf16_bytes(params, stream_indices(H, "bwd", ref=True))),
                        ("bias", O(2), f32_bytes(params, stream_indices(H, "bias", ref=True))),
                        ("normal pass", O(6), bf16_bytes(params, stream_indices(H, "nrm"))),
                        ("directional forward", O(7), bf16_bytes(params, stream_indices(H, "dir_fwd"))),
                        ("directional transposed", O(8), bf16_bytes(params, stream_indices(H, "dir_bwd"))),
                        ("directional bias", O(9), f32_bytes(params, stream_indices(H, "dir_bias")))], n)


def test_refnerf_render_pack(H, params):
    O = H.lnrf_host_pack_offset
    got, n = run_pack("lnrf_refnerf_render_pack", L.lib().lnrf_refnerf_render_packed_bytes, params, False)
    assert n == O(16)
    fwd3 = stream_indices(H, "fwd3", ref=True)[:(O(12) - O(11)) // 2]  # the blob ends the stream behind Dense_8
    check_regions(got, [("split forward", O(11), split_bytes(params, fwd3)),
                        ("bias", O(12), f32_bytes(params, stream_indices(H, "bias", ref=True))),
                        ("split normal pass", O(13), split_bytes(params, stream_indices(H, "nrm"), True)),
                        ("split directional forward", O(14), split_bytes(params, stream_indices(H, "dir_fwd"), True)),
                        ("directional bias", O(15), f32_bytes(params, stream_indices(H, "dir_bias")))], n)
