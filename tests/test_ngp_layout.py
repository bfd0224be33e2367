"""
CPU check of the data layout of the fused InstantNGPModel MLP (csrc/ngp_layout.h, compiled for the host into
liblnrf_layout_host.so): the pack walks of the forward / transposed stream and the bias block, the weight-gradient table of
the persistent backward with its gradient-vector addressing, and the forward chain run on the MFMA emulator of
test_nerf_layout.py against the oracle's bf16-operand InstantNGPModel.  No GPU involved.

enc_dim = L*F covers the support bounds (1, 32), both sides of the switch between one and two k-steps of encoding (16, 17),
and a ragged k-step (2, 6, 17).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import instant_ngp as ONGP
from oracle import model as OM
from test_nerf_layout import HOST_LIB, bf16, mfma_32x32x16

ENC_DIMS = [1, 2, 6, 16, 17, 32]
HIDDEN, DENSITY, DEMB = 64, 16, 24


@pytest.fixture(scope="module")
def H():
    if not os.path.exists(HOST_LIB):
        pytest.skip("liblnrf_layout_host.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(HOST_LIB)
    lib.lnrf_host_ngp_stream_indices.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.lnrf_host_ngp_stream_indices.restype = ctypes.c_int64
    lib.lnrf_host_ngp_pack_offset.restype = ctypes.c_int64
    lib.lnrf_host_ngp_wgrad_owners.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]
    lib.lnrf_host_ngp_wgrad_owners.restype = ctypes.c_int64
    lib.lnrf_host_ngp_parts_plan.argtypes = [ctypes.c_int, ctypes.c_void_p]
    return lib


def ngp_stream_indices(H, stream, enc_dim):
    """Index array of stream 0 forward, 1 transposed, 2 bias block, relative to the first Dense parameter."""
    n = H.lnrf_host_ngp_stream_indices(stream, enc_dim, None)
    assert n > 0
    out = np.full(n, -2, np.int32)
    assert H.lnrf_host_ngp_stream_indices(stream, enc_dim, out.ctypes.data) == n
    return out


def dense_layout(enc_dim):
    """[(kernel offset, fan_in, fan_out, bias offset)] of Dense_0..4 and the Dense parameter count (Flax order)."""
    dims = [(enc_dim, HIDDEN), (HIDDEN, DENSITY), (DEMB + DENSITY, HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, 3)]
    out, off = [], 0
    for fi, fo in dims:
        out.append((off, fi, fo, off + fi * fo))
        off += fi * fo + fo
    return out, off


def chain_shape(enc_dim):
    """(k-steps, 32-row out tiles) of the five forward layers and the five transposed steps, in stream order."""
    ne = 1 if enc_dim <= 16 else 2
    return [(ne, 2), (4, 1), (3, 2), (4, 2), (4, 1)], [(1, 2), (4, 2), (4, 1), (1, 2), (4, 1)]


def counts_of(idx, n):
    assert idx.min() >= -1 and idx.max() < n
    return np.bincount(idx[idx >= 0], minlength=n)


@pytest.mark.parametrize("enc_dim", ENC_DIMS)
def test_forward_stream_and_bias_block_pack_every_parameter_once(H, enc_dim):
    layers, n = dense_layout(enc_dim)
    fwd_shape, _ = chain_shape(enc_dim)
    n_fwd = sum(nk * no for nk, no in fwd_shape)
    fwd = ngp_stream_indices(H, 0, enc_dim).reshape(-1, 512)
    assert fwd.shape[0] == H.lnrf_host_ngp_pack_offset(4) == 48 and n_fwd <= 26 == H.lnrf_host_ngp_pack_offset(5)
    assert (fwd[n_fwd:] == -1).all(), "fragments past the forward stream must be empty"
    bias = ngp_stream_indices(H, 2, enc_dim)
    assert bias.shape == (256,) and H.lnrf_host_ngp_pack_offset(0) == 48 * 1024
    cw, cb = counts_of(fwd.reshape(-1), n), counts_of(bias, n)
    row0 = 0
    for (w, fi, fo, b), (nk, no) in zip(layers, fwd_shape):
        assert (cw[w:b] == 1).all() and (cw[b:b + fo] == 0).all(), "every Dense weight once, no bias in the stream"
        assert (cb[b:b + fo] == 1).all() and (cb[w:b] == 0).all()
        # the layer's rows of the bias block: its biases in order, then padding up to whole 32-row tiles
        assert (bias[row0:row0 + fo] == b + np.arange(fo)).all() and (bias[row0 + fo:row0 + 32 * no] == -1).all()
        row0 += 32 * no
    assert row0 == 256


@pytest.mark.parametrize("enc_dim", ENC_DIMS)
def test_transposed_stream_packs_what_the_input_gradients_need(H, enc_dim):
    layers, n = dense_layout(enc_dim)
    fwd_shape, bwd_shape = chain_shape(enc_dim)
    n_fwd, n_bwd = sum(nk * no for nk, no in fwd_shape), sum(nk * no for nk, no in bwd_shape)
    bwd = ngp_stream_indices(H, 1, enc_dim).reshape(-1, 512)
    fwd = ngp_stream_indices(H, 0, enc_dim).reshape(-1, 512)
    assert (bwd[:n_fwd] == -1).all() and (bwd[n_fwd + n_bwd:] == -1).all()
    assert not ((fwd >= 0) & (bwd >= 0)).any()
    c = counts_of(bwd.reshape(-1), n)
    for l, (w, fi, fo, b) in enumerate(layers):
        k = c[w:b].reshape(fi, fo)
        if l == 2:  # only the rows fed by `out`; d_emb has no parameters upstream
            assert (k[DEMB:] == 1).all() and (k[:DEMB] == 0).all()
        else:
            assert (k == 1).all()
        assert (c[b:b + fo] == 0).all()


@pytest.mark.parametrize("enc_dim", ENC_DIMS)
def test_every_dense_gradient_entry_has_one_owner_per_k_part(H, enc_dim):
    """The persistent backward stores its share of dW with plain stores into one row per (workgroup, k-part), and the
    reduce launch adds `parts` rows per parameter: every Dense entry must be stored exactly once in each of its layer's
    k-part rows and in no other.  A bias entry stored by a tile other than the it == 0 one of its (k-part, out tile) would
    be stored twice, so this also pins the bias sums to the it == 0 tiles."""
    layers, n = dense_layout(enc_dim)
    plan = np.zeros((5, 4), np.int32)
    assert H.lnrf_host_ngp_parts_plan(enc_dim, plan.ctypes.data) == n
    max_parts = H.lnrf_host_ngp_pack_offset(6)
    assert [int(l) for l in plan[:, 0]] == [3, 2, 1, 4, 0], "problem order of the kernel argument"
    for l, lo, hi, parts in plan:
        w, fi, fo, b = layers[l]
        assert (lo, hi) == (w, b + fo) and 1 <= parts <= max_parts
    order = np.argsort(plan[:, 1])
    assert plan[order[0], 1] == 0 and plan[order[-1], 2] == n
    assert (plan[order[1:], 1] == plan[order[:-1], 2]).all(), "the ranges tile the Dense block"

    count = np.zeros((max_parts, n), np.int32)
    assert H.lnrf_host_ngp_wgrad_owners(enc_dim, count.ctypes.data, n) == 0, "a store outside the Dense block"
    for l, lo, hi, parts in plan:
        assert (count[:parts, lo:hi] == 1).all(), f"Dense_{l}: an entry of a k-part row without exactly one owner"
        assert (count[parts:, lo:hi] == 0).all(), f"Dense_{l}: a store into a row the reduce launch does not read"


def emulated_ngp_forward(H, enc_dim):
    """The forward 'program' of ngp_mlp_kernel for one 32-evaluation tile, driven by the exported index arrays and the
    k-slot map only.  -> the emulator's density and rgb and the oracle's."""
    gen = torch.Generator().manual_seed(enc_dim)
    feature_dim = 2 if enc_dim % 2 == 0 else 1
    levels = enc_dim // feature_dim
    grid_sizes = [2 + l % 3 for l in range(levels)]
    table_sizes = [64] * levels  # dense levels (grid^3 <= 64)
    rows, dims = ONGP.ngp_spec(table_sizes, grid_sizes, feature_dim)
    layers, n_dense = dense_layout(enc_dim)
    assert [(fi, fo) for _, fi, fo, _ in layers] == dims
    tables = torch.rand(sum(rows) * feature_dim, generator=gen) * 2 - 1
    dense = torch.zeros(n_dense)
    for w, fi, fo, b in layers:
        dense[w:b] = torch.randn(fi * fo, generator=gen) / fi ** 0.5
        dense[b:b + fo] = torch.randn(fo, generator=gen) * 0.1
    flat = torch.cat([tables, dense]).float()
    x = (torch.rand(32, 3, generator=gen) * 2 - 1).float()
    d = torch.randn(32, 3, generator=gen)
    d = (d / d.norm(dim=-1, keepdim=True)).float()
    bmin, bmax = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    ref_density, ref_rgb, _ = ONGP.ngp_model(flat.double(), x.double(), d.double(), table_sizes, grid_sizes, bmin, bmax,
                                             feature_dim=feature_dim, operand_round=OM.bf16_round)

    # inputs of the MLP, from the oracle's own encoders
    off, feats = 0, []
    for r, t, g in zip(rows, table_sizes, grid_sizes):
        table = flat[off:off + r * feature_dim].double().reshape(r, feature_dim)
        off += r * feature_dim
        feats.append(ONGP.hash_table_encoding(x.double(), table, g, t, torch.tensor(bmin).double(),
                                              torch.tensor(bmax).double()))
    enc = torch.cat(feats, dim=1).numpy()
    d_emb = OM.sinusoidal_emb(d.double(), 4).numpy()
    assert enc.shape == (32, enc_dim) and d_emb.shape == (32, DEMB)

    P = dense.numpy()
    fwd = ngp_stream_indices(H, 0, enc_dim).reshape(-1, 64, 8)
    bias_idx = ngp_stream_indices(H, 2, enc_dim)
    bias = np.where(bias_idx >= 0, P[np.maximum(bias_idx, 0)], 0.0).astype(np.float64)

    def a_frag(g):
        return bf16(np.where(fwd[g] >= 0, P[np.maximum(fwd[g], 0)], 0.0)).astype(np.float64)

    def input_frags(values, nks):  # B fragments of a tensor [32, features]: k slot (ks, h, j) <-> feature hidden_feat
        fr = np.zeros((nks, 64, 8), np.float32)
        for ks in range(nks):
            for lane in range(64):
                for j in range(8):
                    e = H.lnrf_host_hidden_feat(ks, lane >> 5, j)
                    fr[ks, lane, j] = values[lane & 31, e] if e < values.shape[1] else 0.0
        return list(bf16(fr).astype(np.float64))

    cursor = {"frag": 0, "bias": 0}

    def layer(b_frags, no, relu):  # consumes no * len(b_frags) fragments and 32 * no bias rows, in stream order
        nk, outs, frags = len(b_frags), [], []
        for o in range(no):
            acc = np.zeros((64, 16), np.float64)
            for lane in range(64):
                for q in range(16):
                    acc[lane, q] = bias[cursor["bias"] + 32 * o + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)]
            for ks in range(nk):
                acc = mfma_32x32x16(a_frag(cursor["frag"] + o * nk + ks), b_frags[ks], acc)
            outs.append(acc)
            v = np.maximum(acc, 0) if relu else acc  # registers 8s..8s+7 -> B fragment of k-step s of the next layer
            frags += [bf16(v[:, :8]).astype(np.float64), bf16(v[:, 8:]).astype(np.float64)]
        cursor["frag"] += no * nk
        cursor["bias"] += 32 * no
        return outs, frags

    ne = 1 if enc_dim <= 16 else 2
    _, h0 = layer(input_frags(enc, ne), 2, True)
    out1, o16 = layer(h0, 1, False)
    density = np.exp(out1[0][:32, 0])  # feature 0 = register 0 of lanes 0..31
    _, c1 = layer(input_frags(d_emb, 2) + o16[:1], 2, True)
    _, c2 = layer(c1, 2, True)
    out4, _ = layer(c2, 1, False)
    rgb = np.tanh(out4[0][:32, :3])
    assert cursor["frag"] == sum(nk * no for nk, no in chain_shape(enc_dim)[0]) and cursor["bias"] == 256
    return density, rgb, ref_density.numpy()[:, 0], ref_rgb.numpy()


@pytest.mark.parametrize("enc_dim", ENC_DIMS)
def test_emulated_ngp_forward_chain_matches_oracle(H, enc_dim):
    density, rgb, ref_density, ref_rgb = emulated_ngp_forward(H, enc_dim)
    assert np.abs(rgb - ref_rgb).max() < 2e-5
    assert np.abs(density - ref_density).max() < 2e-5
