"""
The four NeRFModel / RefNERFModel weight-packing kernels against blobs built on the host from the index arrays of the
layout library (csrc/nerf_layout.h pack walks, exported by liblnrf_layout_host.so): byte for byte over every region a
kernel writes, no tolerance.  Weights are bf16(params[idx]) with 0 for idx == -1, split streams hold hi = bf16(w) in the even
and lo = bf16(w - float(hi)) in the odd fragments, biases are exact fp32; the region offsets are the library's constants.
The unwritten tail behind a bias block is not compared.
The two InstantNGPModel pack kernels likewise, against the index arrays of csrc/ngp_layout.h (test_ngp_layout.py).
"""
import ctypes

import numpy as np
import pytest
import torch

from learn_nerf import _lib as L
from test_nerf_layout import HOST_LIB, stream_indices
from test_ngp_layout import dense_layout, ngp_stream_indices

pytestmark = pytest.mark.gpu

N_PARAMS = 593_924  # NeRFModel; RefNERFModel's vector is shorter


@pytest.fixture(scope="module")
def H():
    lib = ctypes.CDLL(HOST_LIB)
    lib.lnrf_host_pack_offset.restype = ctypes.c_int64
    lib.lnrf_host_ngp_pack_offset.restype = ctypes.c_int64
    lib.lnrf_host_ngp_stream_indices.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.lnrf_host_ngp_stream_indices.restype = ctypes.c_int64
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


def run_ngp_pack(fn_name, bytes_fn_name, params, enc_dim, dense_offset):
    lib = L.lib()
    desc = L.NgpMlpDesc(enc_dim, 64, 16, 1, 2, 4, dense_offset)
    nbytes = getattr(lib, bytes_fn_name)(ctypes.byref(desc))
    flat = params[:dense_offset + dense_layout(enc_dim)[1]].cuda()
    packed = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    L.check(getattr(lib, fn_name)(ctypes.byref(desc), L.ptr(flat), L.ptr(packed, torch.uint8), L.stream()), fn_name)
    torch.cuda.synchronize()
    return packed.cpu(), nbytes


def ngp_indices(H, stream, enc_dim, dense_offset):
    idx = ngp_stream_indices(H, stream, enc_dim).astype(np.int64)  # relative to the first Dense parameter
    return np.where(idx >= 0, idx + dense_offset, -1)


@pytest.mark.parametrize("dense_offset", [0, 1001])
@pytest.mark.parametrize("enc_dim", [1, 6, 16, 17, 32])
def test_ngp_mlp_pack(H, params, enc_dim, dense_offset):
    O = H.lnrf_host_ngp_pack_offset
    got, n = run_ngp_pack("lnrf_ngp_mlp_pack", "lnrf_ngp_mlp_packed_bytes", params, enc_dim, dense_offset)
    assert n == O(1)
    # one stream of 48 fragments: the forward walk owns the front, the transposed walk what follows (never both)
    stream = np.maximum(ngp_indices(H, 0, enc_dim, dense_offset), ngp_indices(H, 1, enc_dim, dense_offset))
    check_regions(got, [("stream", 0, bf16_bytes(params, stream)),
                        ("bias", O(0), f32_bytes(params, ngp_indices(H, 2, enc_dim, dense_offset)))], n)


@pytest.mark.parametrize("dense_offset", [0, 1001])
@pytest.mark.parametrize("enc_dim", [1, 6, 16, 17, 32])
def test_ngp_mlp_pack_split(H, params, enc_dim, dense_offset):
    O = H.lnrf_host_ngp_pack_offset
    got, n = run_ngp_pack("lnrf_ngp_mlp_pack_split", "lnrf_ngp_mlp_packed_split_bytes", params, enc_dim, dense_offset)
    assert n == O(3)
    fwd = ngp_indices(H, 0, enc_dim, dense_offset)[:O(5) * 512]  # the blob pairs the first 26 fragments
    check_regions(got, [("split forward", 0, split_bytes(params, fwd, True)),
                        ("bias", O(2), f32_bytes(params, ngp_indices(H, 2, enc_dim, dense_offset)))], n)
