"""
CPU checks of tests/nerf_dump_decode.py: the decoders of the forward save and of the gradient dump of the fused NeRFModel
kernels, and the two comparison rules of test_gpu_nerf_stagewise.py.  No GPU involved.

  round trip          decode(encode(t)) == t at tile edges; every byte of a tile's block belongs to exactly one element or
                      is a documented zero / pad region
  against the kernel  the NumPy MFMA emulation of the forward (test_nerf_layout.py) leaves its fragments in a save buffer
                      the way the kernel does (lane (c, hh) of slot F at dump_lane_off); the decoder must return the
                      emulator's activations in feature order, taken from the MFMA result map alone — a decoder that
                      permutes features consistently with its own encoder fails here
  directional dumps   the same for the two dumps of the Ref-NeRF directional block (dir_layouts()): round trips, one owner per
                      bit, the pad k-slots of xin and the empty second slot of dy10 identified, the kernel's fragment order
  the rules           accept the fp32-accumulated CPU result and reject each mutation a 3e-2 relative-L2 gate cannot see
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import nerf_dump_decode as D
from test_nerf_layout import bf16, emulated_forward_chain


@pytest.fixture(scope="module")
def H():
    try:
        lib = D.load_host_lib()
    except FileNotFoundError as e:
        pytest.skip(str(e))
    lib.lnrf_host_sincos_pe.argtypes = [ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    return lib


def rand_bf16(rng, *shape):
    return D.bf16_rne(rng.standard_normal(shape))


def test_bf16_rne_is_one_rounding():
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(100000) * 10.0 ** rng.integers(-6, 6, 100000)).astype(np.float32)
    want = torch.from_numpy(v).to(torch.bfloat16).to(torch.float64).numpy()  # fp32 -> bf16 is a single rounding
    assert (D.bf16_rne(v.astype(np.float64)) == want).all()
    # 1 + 2^-8 + 2^-30 lies above the midpoint of 1 and 1 + 2^-7; rounded to fp32 first it IS the midpoint and the tie goes
    # to the even neighbour 1
    x = 1.0 + 2.0 ** -8 + 2.0 ** -30
    assert D.bf16_rne(x) == 1.0 + 2.0 ** -7 and float(torch.tensor(x, dtype=torch.float64).float().bfloat16()) == 1.0
    assert D.bf16_rne(1.0 + 2.0 ** -8) == 1.0 and D.bf16_rne(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6  # ties to even
    assert D.bf16_trunc(1.0 + 2.0 ** -7 - 2.0 ** -20) == 1.0 and D.bf16_trunc(-1.0 - 2.0 ** -7 + 2.0 ** -20) == -1.0
    bits = np.arange(0x0000, 0x7F80, dtype=np.uint16)  # every finite non-negative bf16, subnormals included
    assert (D.f64_to_bf16_bits(D.bf16_rne(D.bf16_bits_to_f64(bits))) == bits).all()


def random_save(rng, m):
    t = {"x_emb": rand_bf16(rng, m, 60), "z": rand_bf16(rng, m, 256), "d_emb": rand_bf16(rng, m, 24),
         "h": [np.maximum(rand_bf16(rng, m, 256), 0) for _ in range(8)], "h10": np.maximum(rand_bf16(rng, m, 128), 0),
         "mask": [rng.random((m, 256)) < 0.5 for _ in range(8)], "mask10": rng.random((m, 128)) < 0.5}
    return t


def random_grad(rng, m):
    return {"dy": [rand_bf16(rng, m, 256) for _ in range(9)], "dy10": rand_bf16(rng, m, 128), "dlogit": rand_bf16(rng, m),
            "dy11": rand_bf16(rng, m, 3)}


@pytest.mark.parametrize("m", [1, 31, 32, 33, 70])
def test_round_trip(H, m):
    rng = np.random.default_rng(m)
    t = random_save(rng, m)
    for hidden_masks in (True, False):
        buf = D.encode_save(t, m, hidden_masks=hidden_masks)
        assert buf.size == D.padded_tiles(m) * D.layouts()[0].tile_bytes()
        got = D.decode_save(buf, m, hidden_masks=hidden_masks)
        for name in ("x_emb", "z", "d_emb", "h10", "mask10"):
            assert got[name].shape == t[name].shape and (got[name].numpy() == t[name]).all(), name
        for l in range(8):
            assert (got["h"][l].numpy() == t["h"][l]).all(), l
            if hidden_masks:
                assert (got["mask"][l].numpy() == t["mask"][l]).all(), l
            else:
                assert got["mask"][l] is None
        # what the encoder does not write reads back as zero: pad evaluations, unused k-slots, the bit-free half of mask10
        assert all(not v.numpy().any() for v in got["pad"].values())
        assert set(got["pad_slots"]) == {"x_emb", "d_emb"} and all(not v.numpy().any() for v in got["pad_slots"].values())
        assert got["pad"]["x_emb"].shape == (32 * D.padded_tiles(m) - m, 60) and not got["mask10_high"].numpy().any()
    g = random_grad(rng, m)
    buf = D.encode_grad(g, m)
    assert buf.size == D.grad_dump_bytes(m)
    got = D.decode_grad(buf, m)
    for l in range(9):
        assert (got["dy"][l].numpy() == g["dy"][l]).all(), l
    for name in ("dy10", "dlogit", "dy11"):
        assert got[name].shape == g[name].shape and (got[name].numpy() == g[name]).all(), name
    assert all(not v.numpy().any() for v in got["pad"].values())
    assert set(got["pad_slots"]) == {"dy11", "dy10m"} and all(not v.numpy().any() for v in got["zero_slots"].values())
    # a single changed byte anywhere in a tensor's slots changes what is decoded
    buf2 = buf.copy()
    buf2[D.layouts()[1].pos["dy3"][0, 7] * 2] ^= 0x01
    assert (D.decode_grad(buf2, m)["dy"][3].numpy() != g["dy"][3]).sum() == 1


def test_every_byte_has_one_owner_or_is_documented_free(H):
    """Per tile: every bit of the block is one tensor element's or one mask bit's, except (nerf_layout.h) the pad pair of
    x_emb (4 k-slots per evaluation) and of d_emb (8), the upper 8 bytes per lane of the h10 mask (64 of its 128 bits are
    used), of dy11 all but 3 k-slots and its second slot, of dy10m's logit slot all but 1 and its last slot."""
    save, grad = D.layouts()
    S, G = H.lnrf_host_save_slot, H.lnrf_host_grad_slot
    assert save.n_slots == S(6, 0) and grad.n_slots == G(3, 0)
    for lay, free_bytes in ((save, 32 * 2 * (4 + 8) + 64 * 8), (grad, 32 * 2 * 13 + 1024 + 32 * 2 * 15 + 1024)):
        own = lay.bit_owners().reshape(-1, 8)
        assert own.max() == 1, "two elements share a bit"
        assert ((own.sum(1) == 8) | (own.sum(1) == 0)).all(), "a byte is partly owned"
        assert int((own.sum(1) == 0).sum()) == free_bytes
    fb = grad.frag_bytes
    own = grad.bit_owners().reshape(grad.n_slots, fb * 8)
    free_slots = [s for s in range(grad.n_slots) if not own[s].any()]
    assert free_slots == [G(0, 0) + 1, G(1, 0) + 9]  # the documented zero slots
    # and the free regions are exactly what decode_* hands back as pad_slots / zero_slots / mask10_high
    buf = np.full(D.padded_tiles(1) * grad.tile_bytes(), 0xFF, np.uint8)
    got = D.decode_grad(buf, 1)
    n_free = sum(v.numel() * 2 for v in got["pad_slots"].values()) + sum(v.numel() for v in got["zero_slots"].values())
    assert n_free == D.padded_tiles(1) * (32 * 2 * 13 + 1024 + 32 * 2 * 15 + 1024)


def test_decoder_against_the_emulated_kernel(H):
    e = emulated_forward_chain(H)
    save, _ = D.layouts()
    S = H.lnrf_host_save_slot
    n_tiles = D.padded_tiles(32)
    blocks = np.zeros((n_tiles, save.tile_bytes()), np.uint8)

    def put(slot, frag):  # what DumpAddr::store does with one fragment [64 lanes][8 bf16] of tile 0
        bits = D.f64_to_bf16_bits(frag)
        for lane in range(64):
            off = slot * save.frag_bytes + H.lnrf_host_dump_lane_off(slot, lane & 31, lane >> 5)
            blocks[0, off:off + 16] = bits[lane].view(np.uint8)

    def put_mask(slot, accs):  # nerf_layout.h kSaveMask: lane l keeps a uint4 at l * 16, bit 16 o + q = acc reg q of out tile o
        for lane in range(64):
            word = sum(1 << (16 * o + q) for o, acc in enumerate(accs) for q in range(16) if bf16(max(acc[lane, q], 0)) > 0)
            off = slot * save.frag_bytes + lane * 16
            blocks[0, off:off + 16] = np.frombuffer(word.to_bytes(16, "little"), np.uint8)

    def frags_of(accs, relu):
        out = []
        for acc in accs:
            v = np.maximum(acc, 0) if relu else acc
            out += [bf16(v[:, :8]).astype(np.float64), bf16(v[:, 8:]).astype(np.float64)]
        return out

    def feature_order(accs, relu):  # MFMA result map: register q of lane (col, hh) = row (q & 3) + 8 (q >> 2) + 4 hh
        t = np.zeros((32, 32 * len(accs)))
        for o, acc in enumerate(accs):
            for lane in range(64):
                for q in range(16):
                    t[lane & 31, 32 * o + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)] = acc[lane, q]
        return bf16(np.maximum(t, 0) if relu else t).astype(np.float64)

    for ks in range(4):
        put(S(0, 0) + ks, e["xin"][ks])
    for ks in range(2):
        put(S(3, 0) + ks, e["din"][ks])
    want = {"x_emb": bf16(e["x_emb"]).astype(np.float64), "d_emb": bf16(e["d_emb"]).astype(np.float64)}
    for s in range(10):
        accs = e["tiles"][s][:4] if s == 9 else e["tiles"][s]
        slot0 = S(1, s) if s < 8 else (S(2, 0) if s == 8 else S(4, 0))
        for i, f in enumerate(frags_of(accs, relu=s != 8)):
            put(slot0 + i, f)
        if s != 8:
            put_mask(S(5, 0) + (s if s < 8 else 8), accs)
        want["z" if s == 8 else ("h10" if s == 9 else f"h{s}")] = feature_order(accs, relu=s != 8)
    got = D.decode_save(blocks.reshape(-1), 32)
    for name in ("x_emb", "d_emb", "z", "h10"):
        assert (got[name].numpy() == want[name]).all(), name
        assert np.abs(want[name]).max() > 0
    for l in range(8):
        assert (got["h"][l].numpy() == want[f"h{l}"]).all(), l
        assert (got["mask"][l].numpy() == (want[f"h{l}"] > 0)).all(), l
        assert 0.05 < (want[f"h{l}"] > 0).mean() < 0.95
    assert (got["mask10"].numpy() == (want["h10"] > 0)).all()
    # the unused pair of the embeddings is zero in the kernel's fragments, and the decoder says where it looked
    assert not got["pad_slots"]["x_emb"][:32].numpy().any() and not got["pad_slots"]["d_emb"][:32].numpy().any()


def test_decode_is_vectorised(H):
    m = 3000
    rng = np.random.default_rng(1)
    D.layouts()
    sbuf = rng.integers(0, 256, D.padded_tiles(m) * D.layouts()[0].tile_bytes(), dtype=np.uint8)
    sbuf[1::2] &= 0x3F  # keep every bf16 finite
    gbuf = sbuf[:D.grad_dump_bytes(m)].copy()
    t0 = time.perf_counter()
    D.decode_save(sbuf, m)
    D.decode_grad(gbuf, m)
    dt = time.perf_counter() - t0
    print(f"decode_save + decode_grad at m={m}: {dt:.3f} s")
    assert dt < 1.0


# ---- Ref-NeRF directional block -------------------------------------------------------------------------------------------
def random_dir(rng, m):
    save = {"xin": rand_bf16(rng, m, D.DIR_IN), "h9": np.maximum(rand_bf16(rng, m, D.DIR_HIDDEN), 0),
            "mask9": rng.random((m, D.DIR_HIDDEN)) < 0.5}
    return save, {"dy10": rand_bf16(rng, m, 3), "dy9": rand_bf16(rng, m, D.DIR_HIDDEN)}


@pytest.mark.parametrize("m", [1, 31, 32, 33, 70, 257])
def test_dir_round_trip(H, m):
    rng = np.random.default_rng(100 + m)
    save, grad = random_dir(rng, m)
    sl, gl = D.dir_layouts()
    buf = D.encode_dir_save(save, m)
    assert buf.size == D.padded_tiles(m) * sl.tile_bytes()
    got = D.decode_dir_save(buf, m)
    for name in save:
        assert got[name].shape == save[name].shape and (got[name].numpy() == save[name]).all(), name
    assert all(not v.numpy().any() for v in got["pad"].values()) and not got["mask9_high"].numpy().any()
    assert set(got["pad_slots"]) == {"xin"} and not got["pad_slots"]["xin"].numpy().any() and not got["zero_slots"]
    assert got["pad"]["xin"].shape == (32 * D.padded_tiles(m) - m, D.DIR_IN)
    buf = D.encode_dir_grad(grad, m)
    assert buf.size == D.dir_grad_dump_bytes(m)
    got = D.decode_dir_grad(buf, m)
    for name in grad:
        assert got[name].shape == grad[name].shape and (got[name].numpy() == grad[name]).all(), name
    assert all(not v.numpy().any() for v in got["pad"].values())
    assert set(got["pad_slots"]) == {"dy10"} and not got["pad_slots"]["dy10"].numpy().any() and not got["zero_slots"]
    # a single changed byte anywhere in a tensor's slots changes what is decoded
    buf2 = buf.copy()
    buf2[gl.pos["dy9"][m % 32 - 1, 127] * 2 + (m - 1) // 32 * gl.tile_bytes()] ^= 0x01
    assert (D.decode_dir_grad(buf2, m)["dy9"].numpy() != grad["dy9"]).sum() == 1


def test_dir_every_bit_has_one_owner_and_the_pads_are_identified(H):
    """Per tile of the directional dumps every bit is one tensor element's or one mask bit's, except: the 15 k-slots of xin that
    stand for inputs 273..287, the upper 8 bytes per lane of the mask slot (128 of its 256 bits per lane pair are used), and of
    dy10 all but its 3 colour channels: 13 k-slots of its first slot and the whole second slot."""
    save, grad = D.dir_layouts()
    S = H.lnrf_host_dir_slot
    assert save.n_slots == S(3) and grad.n_slots == S(6) and S(7) == -1
    n_pad_in = 16 * save.tensors["xin"].nks - D.DIR_IN
    for lay, free_bytes in ((save, 32 * 2 * n_pad_in + 64 * 8), (grad, 32 * 2 * 13 + save.frag_bytes)):
        own = lay.bit_owners().reshape(-1, 8)
        assert own.max() == 1, "two elements share a bit"
        assert ((own.sum(1) == 8) | (own.sum(1) == 0)).all(), "a byte is partly owned"
        assert int((own.sum(1) == 0).sum()) == free_bytes
    # the pad k-slots of xin are those whose input feature does not exist, all in the last k-step
    hid = np.array([[[H.lnrf_host_hidden_feat(ks, h, j) for j in range(8)] for h in range(2)] for ks in range(save.tensors["xin"].nks)])
    feat = save.tensors["xin"].feat
    assert ((feat == -1) == (hid >= D.DIR_IN)).all() and (feat == -1).sum() == n_pad_in == 15 and (feat[:-1] >= 0).all()
    assert feat[-1, 0, 0] == D.DIR_IN - 1  # the scalar tail load: feature 272 alone in its k-step
    # dy10: lane half 0 keeps channel j in element j (refnerf_dir_bwd_kernel), the second slot carries nothing
    f10 = grad.tensors["dy10"].feat
    assert f10.shape == (2, 2, 8) and (f10[1] == -1).all() and (f10[0, 1] == -1).all() and f10[0, 0].tolist() == [0, 1, 2] + [-1] * 5
    # and the free regions are exactly what the decoders hand back
    n = D.padded_tiles(1)
    got = D.decode_dir_save(np.full(n * save.tile_bytes(), 0xFF, np.uint8), 1)
    assert got["pad_slots"]["xin"].shape == (32 * n, n_pad_in) and (got["pad_slots"]["xin"].numpy() == 0xFFFF).all()
    assert got["mask9_high"].numel() == n * 64 * 8 and got["mask9"].all()
    got = D.decode_dir_grad(np.full(n * grad.tile_bytes(), 0xFF, np.uint8), 1)
    assert got["pad_slots"]["dy10"].shape == (32 * n, 13 + 16) and (got["pad_slots"]["dy10"].numpy() == 0xFFFF).all()
    second = grad.tensors["dy10"].slot0 + 1
    assert second == S(4) + 1 == S(5) - 1
    blocks = np.zeros((n, grad.tile_bytes()), np.uint8)
    blocks[:, second * grad.frag_bytes:(second + 1) * grad.frag_bytes] = 0xFF
    got = D.decode_dir_grad(blocks.reshape(-1), 1)
    assert (got["pad_slots"]["dy10"].numpy() != 0).sum() == 32 * n * 16 and not got["dy10"].numpy().any() and not got["dy9"].numpy().any()


def test_dir_decoder_against_the_fragment_order_of_the_kernel(H):
    """refnerf_dir_fwd_kernel builds its input fragments from row[16 ks + 4 h + (0..3)] and row[16 ks + 8 + 4 h + (0..3)] and
    stores fragment ks of lane (c, h) at dump_lane_off(slot, c, h); the decoder must hand the row back in feature order"""
    save, _ = D.dir_layouts()
    S = H.lnrf_host_dir_slot
    rng = np.random.default_rng(9)
    rows = rand_bf16(rng, 32, D.DIR_IN)
    padded = np.zeros((32, 16 * save.tensors["xin"].nks))
    padded[:, :D.DIR_IN] = rows
    blocks = np.zeros((D.padded_tiles(32), save.tile_bytes()), np.uint8)
    for ks in range(save.tensors["xin"].nks):
        for c in range(32):
            for h in range(2):
                frag = np.concatenate([padded[c, 16 * ks + 4 * h:16 * ks + 4 * h + 4], padded[c, 16 * ks + 8 + 4 * h:16 * ks + 12 + 4 * h]])
                off = (S(0) + ks) * save.frag_bytes + H.lnrf_host_dump_lane_off(S(0) + ks, c, h)
                blocks[0, off:off + 16] = D.f64_to_bf16_bits(frag).view(np.uint8)
    got = D.decode_dir_save(blocks.reshape(-1), 32)
    assert (got["xin"].numpy() == rows).all() and not got["pad_slots"]["xin"].numpy().any()


# ---- the rules ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_case():
    """random ReLU activations x lecun-normal weights + bias, K = 256: operands, float64 reference, delta, fp32 CPU result"""
    gen = torch.Generator().manual_seed(3)
    a = torch.relu(torch.randn(1000, 256, generator=gen)).bfloat16()
    w = (torch.randn(256, 256, generator=gen) / 16).bfloat16()
    b = (torch.randn(256, generator=gen) * 0.1).float()
    ref = a.double() @ w.double() + b.double()
    delta = D.dot_delta(256, (a.double().abs() @ w.double().abs() + b.double().abs()).numpy())
    cpu = (a.float() @ w.float() + b).double().numpy()
    return ref.numpy(), delta, cpu


def test_check_rounded_accepts_fp32_and_rejects_mutations(dense_case):
    ref, delta, cpu = dense_case
    got = D.bf16_rne(np.maximum(cpu, 0))
    n_allow, n_diff = D.check_rounded(got, ref, delta, relu=True, what="fp32 CPU")
    assert 0 < n_allow < 0.5 * got.size and n_diff < 1e-3 * got.size
    D.check_cap(n_diff, got.size, n_diff / got.size)
    assert D.needed_share_of_delta(got, ref, delta, relu=True) < 1.0
    # without the ReLU (z, dy8)
    D.check_rounded(D.bf16_rne(cpu), ref, delta, what="fp32 CPU, linear")

    # one bf16 ulp on one element that is not near a boundary
    lo, hi = D.bf16_rne(np.maximum(ref - delta, 0)), D.bf16_rne(np.maximum(ref + delta, 0))
    ev, ft = (int(v) for v in np.argwhere((lo == hi) & (got > 0))[17])
    one = got.copy()
    one[ev, ft] = float(D._bf16_of_key(D._bf16_key(one[ev:ev + 1, ft]) + 1)[0])
    with pytest.raises(AssertionError, match=f"evaluation {ev} feature {ft}"):
        D.check_rounded(one, ref, delta, relu=True, what="one ulp")
    # truncation instead of round-to-nearest in the epilogue
    with pytest.raises(AssertionError):
        D.check_rounded(D.bf16_trunc(np.maximum(cpu, 0)), ref, delta, relu=True, what="truncation")
    # two features swapped
    sw = got.copy()
    sw[:, [5, 6]] = sw[:, [6, 5]]
    with pytest.raises(AssertionError):
        D.check_rounded(sw, ref, delta, relu=True, what="swapped features")
    # a ReLU that lets a negative value through, and one that cuts a positive one
    neg = got.copy()
    ev, ft = (int(v) for v in np.argwhere(ref + delta < 0)[3])
    neg[ev, ft] = D.bf16_rne(ref[ev, ft])
    with pytest.raises(AssertionError):
        D.check_rounded(neg, ref, delta, relu=True, what="leaky relu")
    # the cap: the allowance alone would let a kernel pick the wrong neighbour everywhere inside it
    wrong = np.where(lo != hi, np.where(got == lo, hi, lo), got)
    _, n_wrong = D.check_rounded(wrong, ref, delta, relu=True, what="always the other neighbour")
    with pytest.raises(AssertionError, match="cap"):
        D.check_cap(n_wrong, got.size, n_diff / got.size, what="always the other neighbour")


def test_check_accumulated_accepts_fp32_and_rejects_mutations():
    gen = torch.Generator().manual_seed(4)
    m = 1000
    x = torch.relu(torch.randn(m + 1, 256, generator=gen)).bfloat16()
    dy = (torch.randn(m + 1, 128, generator=gen) * (torch.rand(m + 1, 128, generator=gen) < 0.5)).bfloat16()
    xd, yd = x.double(), dy.double()
    ref, s = (xd[:m].T @ yd[:m]).numpy(), (xd[:m].abs().T @ yd[:m].abs()).numpy()
    got = (x[:m].float().T @ dy[:m].float()).numpy()
    assert D.check_accumulated(got, ref, m + 64, s, what="dW, fp32 CPU") < 0.1
    bref, bs = yd[:m].sum(0).numpy(), yd[:m].abs().sum(0).numpy()
    bgot = dy[:m].float().sum(0).numpy()
    D.check_accumulated(bgot, bref, m + 64, bs, what="db, fp32 CPU")
    # one of the m evaluations left out of the sum
    with pytest.raises(AssertionError):
        D.check_accumulated(got, ref - np.outer(xd[123], yd[123]), m + 64, s, what="dW, one evaluation dropped")
    with pytest.raises(AssertionError):
        D.check_accumulated(bgot, bref - yd[123].numpy(), m + 64, bs, what="db, one evaluation dropped")
    # a pad column (evaluation m of the ragged last tile) added
    with pytest.raises(AssertionError):
        D.check_accumulated(got, ref + np.outer(xd[m], yd[m]), m + 64, s, what="dW, pad column added")
    with pytest.raises(AssertionError):
        D.check_accumulated(bgot, bref + yd[m].numpy(), m + 64, bs, what="db, pad column added")
    # one element of 256 x 128 holds its neighbour's sum
    one = got.copy()
    one[200, 100] = got[200, 101]
    with pytest.raises(AssertionError, match=r"element \(200, 100\)"):
        D.check_accumulated(one, ref, m + 64, s, what="dW, one element")
