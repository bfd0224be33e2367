"""
CPU check of the fused-kernel data layout (csrc/nerf_layout.h, compiled for the host into
liblnrf_layout_host.so): the weight packing, the k-slot <-> feature permutations, the stage/consumption
order and the positional-encoding sincos are exercised with a NumPy emulation of
v_mfma_f32_32x32x16_bf16 (operand / accumulator lane maps from the CDNA4 guide) and must reproduce the
oracle's bf16-operand NeRFModel forward.  No GPU involved.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "learn-nerf_amd", "lib", "liblnrf_layout_host.so")


@pytest.fixture(scope="module")
def H():
    if not os.path.exists(HOST_LIB):
        pytest.skip("liblnrf_layout_host.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(HOST_LIB)
    lib.lnrf_host_sincos_pe.argtypes = [ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    return lib


def bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def mfma_32x32x16(a_frag, b_frag, acc):
    """D = A B + C with the gfx950 lane maps: A/B frag [64 lanes][8], acc [64 lanes][16]."""
    A = np.zeros((32, 16), np.float64)
    B = np.zeros((16, 32), np.float64)
    for lane in range(64):
        r, h = lane & 31, lane >> 5
        A[r, 8 * h:8 * h + 8] = a_frag[lane]
        B[8 * h:8 * h + 8, r] = b_frag[lane]
    D = A @ B
    out = acc.copy()
    for lane in range(64):
        col, hh = lane & 31, lane >> 5
        for q in range(16):
            out[lane, q] += D[(q & 3) + 8 * (q >> 2) + 4 * hh, col]
    return out


def test_stream_sizes_and_consumption_order(H):
    assert H.lnrf_host_fwd_frags() == 1200 and H.lnrf_host_bwd_frags() == 1120 and H.lnrf_host_bias_floats() == 2496
    assert H.lnrf_host_fwd_used() == 1186
    seq = [H.lnrf_host_fwd_seq(c) for c in range(1186)]
    assert seq == sorted(seq) and len(set(seq)) == 1186 and seq[-1] < 1200
    assert seq[1088 - 6 + 0] == 1088 - 6  # no gap before the padded L10m layer ...
    # ... but the 6 padding fragments after its 90 are skipped
    c10 = H.lnrf_host_fwd_layer_info(10, 4)
    assert H.lnrf_host_fwd_seq(c10) == H.lnrf_host_fwd_layer_info(10, 2) == 1184
    bseq = [H.lnrf_host_bwd_seq(c) for c in range(1100)]
    assert bseq == sorted(bseq) and bseq[4] == 16  # Dense_11^T uses 4 fragments of its 16-fragment stage


def test_split_precision_stream_order(H):
    """bf16x3 render stream: [hi, lo] fragment pairs in forward order; the weight ring publishes one 16-fragment
    stage per barrier, so consumption must be monotone and must enter EVERY stage at its first fragment."""
    n, used = H.lnrf_host_fwd3_frags(), H.lnrf_host_fwd3_used()
    assert n == 2384 and n % 16 == 0 and used == 2 * 1186
    seq = [H.lnrf_host_fwd3_seq(c) for c in range(used)]
    assert seq == sorted(seq) and len(set(seq)) == used and seq[-1] < n
    entered = [g // 16 for g in seq if g % 16 == 0]
    assert entered == list(range(n // 16)), "a stage would be skipped or entered mid-way"
    # pair c (hi, lo) of layer s sits at fwd3_base(s) + 2 * (index inside the layer), i.e. mirrors fwd_seq
    for s in range(11):
        c0 = H.lnrf_host_fwd_layer_info(s, 4)
        assert H.lnrf_host_fwd3_seq(2 * c0) == H.lnrf_host_fwd3_base(s)
        assert H.lnrf_host_fwd3_seq(2 * c0 + 1) == H.lnrf_host_fwd3_base(s) + 1


def test_every_weight_is_packed_exactly_once(H):
    counts = np.zeros(593_924, np.int32)
    for g in range(1200):
        for lane in range(64):
            for j in range(8):
                idx = H.lnrf_host_fwd_weight_index(g, lane, j)
                if idx >= 0:
                    counts[idx] += 1
    for i in range(2496):
        idx = H.lnrf_host_fwd_bias_index(i)
        if idx >= 0:
            counts[idx] += 1
    assert counts.min() == 1 and counts.max() == 1, "forward stream + bias block must cover every parameter once"
    # transposed stream: every kernel that needs an input gradient, once; Dense_0 and the x_emb/d_emb rows never
    bcounts = np.zeros(593_924, np.int32)
    for g in range(1120):
        for lane in range(64):
            for j in range(8):
                idx = H.lnrf_host_bwd_weight_index(g, lane, j)
                if idx >= 0:
                    bcounts[idx] += 1
    dims = OM.nerf_layer_dims()
    off = 0
    for l, (fi, fo) in enumerate(dims):
        k = bcounts[off:off + fi * fo].reshape(fi, fo)
        if l == 0:
            assert k.sum() == 0
        elif l in (5, 10):
            assert (k[:256] == 1).all() and k[256:].sum() == 0
        else:
            assert (k == 1).all()
        assert bcounts[off + fi * fo:off + fi * fo + fo].sum() == 0
        off += fi * fo + fo


def test_sincos_pe_accuracy(H):
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(20000):
        r = np.float32(rng.uniform(-1.8, 1.8) * 2 ** rng.integers(0, 10))
        s, c = ctypes.c_float(), ctypes.c_float()
        H.lnrf_host_sincos_pe(r, ctypes.byref(s), ctypes.byref(c))
        worst = max(worst, abs(s.value - np.sin(np.float64(r))), abs(c.value - np.cos(np.float64(r))))
    assert worst < 2e-7


def test_dump_lane_offsets_are_a_permutation_and_conflict_free(H):
    for slot in (0, 1, 7):
        offs = sorted(H.lnrf_host_dump_lane_off(slot, c, hh) for c in range(32) for hh in range(2))
        assert offs == list(range(0, 1024, 16))
    # transposed read of the weight-gradient kernel: 32 lanes (2 fragments x 4 rows x 4 pieces) -> 64 distinct banks
    for c0 in (0, 8, 20):
        banks = set()
        for frag in range(2):
            for qp in range(4):
                for p in range(4):
                    off = H.lnrf_host_dump_lane_off(frag, c0 + qp, p & 1) + 8 * (p >> 1) + 1024 * frag
                    banks.update({(off // 4) % 64, (off // 4 + 1) % 64})
        assert len(banks) == 64


def emulated_forward_chain(H):
    """The forward 'program' of nerf_fwd_kernel for one 32-evaluation tile with the real packing maps.  -> the emulator's
    density and rgb, the oracle's, and `tiles`: per stream layer the accumulator tiles [out tile][64 lanes][16 registers]
    (test_nerf_dump_decode_cpu.py places them in a save buffer), plus the embedding fragments and inputs."""
    gen = torch.Generator().manual_seed(0)
    dims = OM.nerf_layer_dims()
    flat = OM.lecun_normal_init(dims, gen)
    off = 0
    for fi, fo in dims:
        off += fi * fo
        flat[off:off + fo] = torch.randn(fo, generator=gen) * 0.1
        off += fo
    x = (torch.rand(32, 3, generator=gen) * 2 - 1).float()
    d = torch.randn(32, 3, generator=gen)
    d = (d / d.norm(dim=-1, keepdim=True)).float()
    P = flat.numpy()

    def a_frag(g):
        f = np.zeros((64, 8), np.float32)
        for lane in range(64):
            for j in range(8):
                idx = H.lnrf_host_fwd_weight_index(g, lane, j)
                f[lane, j] = P[idx] if idx >= 0 else 0.0
        return bf16(f).astype(np.float64)

    bias = np.array([P[i] if (i := H.lnrf_host_fwd_bias_index(k)) >= 0 else 0.0 for k in range(2496)], np.float64)
    xe = OM.sinusoidal_emb(x.double(), 10).numpy()
    de = OM.sinusoidal_emb(d.double(), 4).numpy()

    def emb_frags(emb, feat, nks):
        fr = np.zeros((nks, 64, 8), np.float32)
        for ks in range(nks):
            for lane in range(64):
                c, h = lane & 31, lane >> 5
                for j in range(8):
                    e = feat(ks, h, j)
                    fr[ks, lane, j] = emb[c, e] if e >= 0 else 0.0
        return bf16(fr).astype(np.float64)

    xin = emb_frags(xe, H.lnrf_host_xemb_feat, 4)
    din = emb_frags(de, H.lnrf_host_demb_feat, 2)

    def layer(s, b_frags, relu):
        nk, no, base, bias0 = (H.lnrf_host_fwd_layer_info(s, w) for w in range(4))
        outs = []
        for o in range(no):
            acc = np.zeros((64, 16), np.float64)
            for lane in range(64):
                hh = lane >> 5
                for q in range(16):
                    acc[lane, q] = bias[bias0 + 32 * o + (q & 3) + 8 * (q >> 2) + 4 * hh]
            for ks in range(nk):
                acc = mfma_32x32x16(a_frag(base + o * nk + ks), b_frags[ks], acc)
            outs.append(acc)
        frags = []
        for acc in outs:  # registers 8s..8s+7 -> B-frag of k-step s of the next layer
            v = np.maximum(acc, 0) if relu else acc
            frags += [bf16(v[:, :8]).astype(np.float64), bf16(v[:, 8:]).astype(np.float64)]
        return outs, frags

    tiles = {}
    tiles[0], act = layer(0, list(xin), True)
    for s in (1, 2, 3, 4):
        tiles[s], act = layer(s, act, True)
    tiles[5], act = layer(5, act + list(xin), True)
    for s in (6, 7):
        tiles[s], act = layer(s, act, True)
    tiles[8], z = layer(8, act, False)
    outs, h10 = layer(9, z + list(din), True)
    tiles[9] = outs
    logit = outs[4][:32, 0]  # row 0 of out-tile 4 lives in register 0 of lanes 0..31
    density = np.logaddexp(logit, 0.0)
    outs11, _ = layer(10, h10[:8], False)
    rgb = np.tanh(outs11[0][:32, :3])
    rd, rr, _ = OM.nerf_mlp(flat.double(), x.double(), d.double(), operand_round=OM.bf16_round)
    return dict(density=density, rgb=rgb, ref_density=rd.numpy()[:, 0], ref_rgb=rr.numpy(), tiles=tiles, xin=xin, din=din,
                x_emb=xe, d_emb=de)


def test_emulated_forward_chain_matches_oracle(H):
    """Run the forward 'program' of nerf_fwd_kernel for one 32-evaluation tile with the real packing maps."""
    e = emulated_forward_chain(H)
    assert np.abs(e["rgb"] - e["ref_rgb"]).max() < 2e-5
    assert np.abs(e["density"] - e["ref_density"]).max() < 2e-5


def test_slot_orders_keep_the_merged_weight_gradient_operands_adjacent(H):
    """nerf_layout.h: the weight-gradient problems [z | d_emb] x dy10m and x_emb x [dy0 | dy5] read ONE run of slots per
    operand, and the head-with-weights experiment one run of 26 (z, d_emb, h10): the slot orders must keep those
    neighbours, every tensor on an even slot (fragment pairs / the parity swizzle of dump_lane_off), nothing overlapping."""
    S, G = H.lnrf_host_save_slot, H.lnrf_host_grad_slot
    assert S(3, 0) == S(2, 0) + 16 and S(4, 0) == S(3, 0) + 2          # z, d_emb, h10
    assert S(1, 0) == S(0, 0) + 4 and S(2, 0) == S(1, 7) + 16           # x_emb, h0..h7, z
    assert S(5, 0) == S(4, 0) + 8 and S(6, 0) == S(5, 0) + 9 == 167
    assert all(S(w, a) % 2 == 0 for w, a in [(0, 0), (2, 0), (3, 0), (4, 0)] + [(1, l) for l in range(8)])
    dy = [G(2, l) for l in range(9)]
    assert G(2, 5) == G(2, 0) + 16                                       # dy5 right behind dy0
    assert sorted(dy) == list(range(G(1, 0) + 10, G(3, 0), 16)) and all(v % 2 == 0 for v in dy)
    assert G(0, 0) == 0 and G(1, 0) == 2 and G(3, 0) == 156


WGRAD_LISTS = {"split": 0, "ls_finish": 1, "ref_trunk": 2, "ref_normal": 3, "ref_dir": 4}


def _expected_owners(which):
    """0/1 per entry of the gradient vector: what the caller of that list is documented to add to (include/lnrf.h)."""
    n = 593_924
    want = np.zeros(n, np.int32)
    off = 0
    kernels, biases = [], []
    for fi, fo in OM.nerf_layer_dims():
        kernels.append((off, fi, fo))
        biases.append((off + fi * fo, fo))
        off += fi * fo + fo
    assert off == n

    def kernel(l, row0=0, row1=None):
        o, fi, fo = kernels[l]
        want[o + row0 * fo:o + (fi if row1 is None else row1) * fo] = 1

    def bias(l):
        o, fo = biases[l]
        want[o:o + fo] = 1

    if which == "split":  # everything
        want[:] = 1
    elif which == "ls_finish":  # the complement of what the pipeline owns: Dense_1..8 kernel rows 0..255 and biases
        want[:] = 1
        for l in range(1, 9):
            o, fi, fo = kernels[l]
            want[o:o + 256 * fo] = 0
            want[biases[l][0]:biases[l][0] + fo] = 0
    elif which == "ref_trunk":  # behind the same pipeline: Dense_0 and the x_emb rows of Dense_5
        kernel(0)
        bias(0)
        kernel(5, 256)
    elif which == "ref_normal":  # d L / d Dense_0..8 through n_raw: kernels only
        for l in range(9):
            kernel(l)
    return want


@pytest.mark.parametrize("n_tiles", [8, 48, 1 << 16])
@pytest.mark.parametrize("which", list(WGRAD_LISTS))
def test_every_gradient_entry_has_exactly_one_owner(H, which, n_tiles):
    """nerf_wgrad.h: the fold of a weight-gradient launch adds to the gradient vector with a plain read-modify-write, so
    every entry a caller is responsible for must belong to exactly one (problem, wave, tile, lane, register) and no other
    entry to any.  Walks the production problem lists and index arithmetic (the code nerf_wgrad_reduce_kernel runs)."""
    C = H.lnrf_host_wgrad_const
    capacity, max_tiles, max_to, n_params = C(0), C(1), C(2), C(3)
    assert n_params == 593_924
    lid = WGRAD_LISTS[which]
    info = np.zeros((13, 6), np.int32)
    H.lnrf_host_wgrad_list.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    n_prob = H.lnrf_host_wgrad_list(lid, n_tiles, info.ctypes.data)
    assert n_prob == {"split": 13, "ls_finish": 3, "ref_trunk": 1, "ref_normal": 9, "ref_dir": 2}[which]
    info = info[:n_prob]
    # workgroup ranges: contiguous from 0, none empty, within the slab region; shapes within a slab
    assert (info[:, 1] >= 1).all()
    assert info[0, 0] == 0 and (info[1:, 0] == info[:-1, 0] + info[:-1, 1]).all()
    assert info[:, 1].sum() <= capacity
    assert (info[:, 2] <= max_tiles).all() and (info[:, 3] <= max_to).all()
    if which == "ls_finish":
        assert (info[:, 5] == 1).all(), "nerf_ls_fold_kernel must carry every shape of the finish phase"
    if which == "ref_normal":
        assert (info[:, 4] == 0).all()

    # RefNERFModel's vector is longer than NeRFModel's behind Dense_8: count over a vector that holds both
    n = max(n_params, C(7) + 3) + 1024
    counts = np.zeros(n, np.int32)
    H.lnrf_host_wgrad_owners.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    H.lnrf_host_wgrad_owners.restype = ctypes.c_int64
    assert H.lnrf_host_wgrad_owners(lid, n_tiles, counts.ctypes.data, n) == 0
    if which == "ref_dir":
        w9, b9, w10, b10 = C(4), C(5), C(6), C(7)
        assert (b9, w10, b10) == (w9 + 273 * 128, w9 + 273 * 128 + 128, w9 + 273 * 128 + 128 + 128 * 3)
        want = np.zeros(n, np.int32)
        want[w9:b10 + 3] = 1
    else:
        want = np.concatenate([_expected_owners(which), np.zeros(n - n_params, np.int32)])
    assert want.sum() > 0
    missing, twice, stray = (counts == 0) & (want == 1), counts > 1, (counts > 0) & (want == 0)
    assert not missing.any() and not twice.any() and not stray.any(), (
        f"{which}: {missing.sum()} unowned, {twice.sum()} owned more than once, {stray.sum()} outside the caller's entries")


STREAMS = {"fwd": 0, "bwd": 1, "fwd3": 2, "bias": 3, "nrm": 4, "dir_fwd": 5, "dir_bwd": 6, "dir_bias": 7}


def stream_indices(H, stream, ref=False):
    """The index array of a whole stream through the pack walks of nerf_layout.h (what the pack kernels call)."""
    H.lnrf_host_stream_indices.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    H.lnrf_host_stream_indices.restype = ctypes.c_int64
    n = H.lnrf_host_stream_indices(STREAMS[stream], int(ref), None)
    assert n > 0
    out = np.full(n, -2, np.int32)
    assert H.lnrf_host_stream_indices(STREAMS[stream], int(ref), out.ctypes.data) == n
    return out


def test_stream_index_arrays_are_the_per_element_exports(H):
    fwd, bwd, bias = stream_indices(H, "fwd"), stream_indices(H, "bwd"), stream_indices(H, "bias")
    assert fwd.shape == (1200 * 512,) and bwd.shape == (1120 * 512,) and bias.shape == (2496,)
    rng = np.random.default_rng(0)
    for e in rng.integers(0, fwd.size, 2000):
        assert fwd[e] == H.lnrf_host_fwd_weight_index(int(e >> 9), int((e >> 3) & 63), int(e & 7))
    for e in rng.integers(0, bwd.size, 2000):
        assert bwd[e] == H.lnrf_host_bwd_weight_index(int(e >> 9), int((e >> 3) & 63), int(e & 7))
    assert all(bias[i] == H.lnrf_host_fwd_bias_index(i) for i in range(2496))


def test_split_stream_mirrors_the_forward_stream(H):
    """Fragments 2p (hi) and 2p + 1 (lo) of a layer of the split stream both carry the indices of forward fragment p of that
    layer; the stage-alignment padding of either stream is -1."""
    fwd = stream_indices(H, "fwd").reshape(1200, 512)
    fwd3 = stream_indices(H, "fwd3").reshape(2384, 512)
    covered = np.zeros(2384, bool)
    for s in range(11):
        nk, no, base = (H.lnrf_host_fwd_layer_info(s, w) for w in range(3))
        base3 = H.lnrf_host_fwd3_base(s)
        for p in range(nk * no):
            assert (fwd3[base3 + 2 * p] == fwd[base + p]).all() and (fwd3[base3 + 2 * p + 1] == fwd[base + p]).all()
            covered[base3 + 2 * p:base3 + 2 * p + 2] = True
        end = H.lnrf_host_fwd_layer_info(s + 1, 2) if s < 10 else 1200
        assert (fwd[base + nk * no:end] == -1).all()
    assert (fwd3[~covered] == -1).all() and (~covered).sum() == 2384 - 2 * 1186


def test_ref_nerf_restriction_keeps_the_trunk_and_zeroes_the_rest(H):
    """RefNERFModel's blobs: forward stream layers <= 8, transposed stream layers >= 2 (Dense_8..1^T) and their biases as in
    the unrestricted maps, -1 everywhere else."""
    fwd_end = H.lnrf_host_fwd_layer_info(9, 2) * 512    # first element of stream layer 9
    bwd_start = H.lnrf_host_bwd_layer_info(2, 2) * 512   # first element of transposed layer 2
    bias_end = H.lnrf_host_fwd_layer_info(9, 3)
    fwd3_end = H.lnrf_host_fwd3_base(9) * 512
    for stream, lo, hi in [("fwd", 0, fwd_end), ("bwd", bwd_start, 1120 * 512), ("bias", 0, bias_end), ("fwd3", 0, fwd3_end)]:
        full, ref = stream_indices(H, stream), stream_indices(H, stream, ref=True)
        assert 0 <= lo < hi <= full.size
        assert (ref[lo:hi] == full[lo:hi]).all(), stream
        assert (ref[:lo] == -1).all() and (ref[hi:] == -1).all(), stream
        assert (full[:lo] >= 0).any() or lo == 0
        assert (full[hi:] >= 0).any() or hi == full.size
