"""
Decoders of the two dumps the fused NeRFModel kernels leave in memory, and the two comparison rules of the stage-wise
tests (test_gpu_nerf_stagewise.py, test_nerf_dump_decode_cpu.py).  A plain module: importing it collects nothing.

  forward save   lnrf_nerf_mlp_fwd / _fwd_ls with a save buffer: x_emb, h0..h7, z, d_emb, h10 and the ReLU masks
  gradient dump  front of the scratch of lnrf_nerf_mlp_bwd_chain / _bwd_ls: dy11, dy10m (Dense_10 outputs + the
                 density-logit slot), dy8..dy0

Both are tile-major [tile][slot][1 KiB fragment]; a fragment holds one k-step (16 features) of 32 evaluations, lane
(c, hh) keeping its 8 bf16 at dump_lane_off(slot, c, hh).  Every slot number, slots-per-tile, lane offset and
k-slot <-> feature map is read from liblnrf_layout_host.so (csrc/nerf_layout.h compiled for the host); this file holds
tensor widths only.  The maps of dy11 and dy10m come from the transposed weight stream itself: k-slot (h, j) of k-step ks
carries the output feature whose weight bwd_weight_index() puts there.

A dump is described by a list of TensorMap (bf16 tensors) and MaskMap (ReLU-mask slots).  The Ref-NeRF directional block
(lnrf_refnerf_dir_fwd / _dir_bwd, csrc/refnerf_fused.hip) leaves two more dumps of the same form, dir_layouts():

  directional save           xin (the 273 inputs as bf16, 18 k-steps, k-slots 273..287 zero), h9 = relu(Dense_9) (8), mask9
  directional gradient dump  front of the scratch of lnrf_refnerf_dir_bwd: dy10 (2 slots, the second all zero; k-slot map
                             from the Dense_10^T rows of the transposed directional stream), dy9 (8)
"""
import ctypes
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "learn-nerf_amd", "lib", "liblnrf_layout_host.so")

# tensor widths (model.py:35-40, default shape) and the Flax parameter vector built from them
X_EMB, D_EMB, HIDDEN, COLOR = 60, 24, 256, 128
DENSE_DIMS = [(X_EMB, HIDDEN)] + [(HIDDEN, HIDDEN)] * 4 + [(HIDDEN + X_EMB, HIDDEN)] + [(HIDDEN, HIDDEN)] * 3 + \
             [(HIDDEN, 1), (HIDDEN + D_EMB, COLOR), (COLOR, 3)]
DIR_IN, DIR_HIDDEN = 273, 128  # RefNERFModel's directional block: Dense_9 273 -> 128 relu, Dense_10 128 -> 3
U23 = 2.0 ** -23  # unit roundoff of a chopping fp32 accumulator; also covers round-to-nearest (2^-24)


def dense_offsets():
    """[(kernel offset, bias offset, fan_in, fan_out)] of Dense_0..11 in the flat parameter vector"""
    out, off = [], 0
    for fi, fo in DENSE_DIMS:
        out.append((off, off + fi * fo, fi, fo))
        off += fi * fo + fo
    return out


N_PARAMS = dense_offsets()[-1][1] + 3


# ---- bf16 -------------------------------------------------------------------------------------------------------------
def bf16_bits_to_f64(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f64_to_bf16_bits(x):
    """bits of values that ARE bf16 numbers (the encoders' inputs); anything else is an error"""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    u = f.view(np.uint32)
    assert not (u & 0xFFFF).any() and (f.astype(np.float64) == np.asarray(x, dtype=np.float64)).all(), "not bf16 values"
    return (u >> 16).astype(np.uint16)


def bf16_rne(x):
    """float64 -> nearest bf16 (ties to even) as float64, in ONE rounding (through float32 it would be two)"""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)  # |x| = f 2^e, f in [0.5, 1): 8 significant bits -> quantum 2^(e - 8); subnormals 2^-133
    q = np.ldexp(1.0, np.maximum(e - 8, -133))
    return np.rint(x / q) * q


def bf16_trunc(x):
    """float64 -> bf16 by chopping (the mutation the tests must catch)"""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    q = np.ldexp(1.0, np.maximum(e - 8, -133))
    return np.trunc(x / q) * q


def _bf16_key(v):
    """order-preserving integer of a bf16 value: neighbours differ by 1, the two zeros coincide"""
    b = f64_to_bf16_bits(v).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def _bf16_of_key(k):
    k = np.asarray(k, dtype=np.int64)
    return np.sign(k) * bf16_bits_to_f64(np.abs(k).astype(np.uint16))


# ---- layout -----------------------------------------------------------------------------------------------------------
class TensorMap:
    """A bf16 tensor of a dump: nks consecutive slots from slot0; feat[ks, h, j] = feature of k-slot (h, j), -1 = unused."""

    def __init__(self, name, slot0, feat, width):
        self.name, self.slot0, self.feat, self.width = name, slot0, np.asarray(feat, np.int64), width
        self.nks = self.feat.shape[0]
        valid = self.feat[self.feat >= 0]
        assert sorted(valid.tolist()) == list(range(width)), f"{name}: the k-slots do not carry every feature once"


class MaskMap:
    """A ReLU-mask slot: bit[ks, j] of the 128 bits lane (c, hh) keeps at lane * 16 <-> feature feat[ks, hh, j]."""

    def __init__(self, name, slot, feat, bit, width):
        self.name, self.slot, self.feat, self.bit, self.width = name, slot, np.asarray(feat, np.int64), np.asarray(bit), width


class DumpLayout:
    """Index arrays of one dump: for a tile's block of n_slots fragments viewed as uint16[n_slots * 512],
    pos[name][c, f] = where evaluation c of the tile keeps feature f; pad[name][c, :] = its unused k-slots."""

    def __init__(self, lib, n_slots, tensors, masks):
        self.frag_bytes, self.cols = lib.lnrf_host_dump_info(0), lib.lnrf_host_dump_info(1)
        self.n_slots, self.tensors, self.masks = n_slots, {t.name: t for t in tensors}, {k.name: k for k in masks}
        half = self.frag_bytes // 2  # uint16 per fragment
        c = np.arange(self.cols)
        self.pos, self.pad, self.mask_pos = {}, {}, {}
        for t in tensors:
            pos = np.full((self.cols, t.width), -1, np.int64)
            pad = []
            for ks in range(t.nks):
                slot = t.slot0 + ks
                for h in range(2):
                    lane_off = np.array([lib.lnrf_host_dump_lane_off(slot, int(ci), h) for ci in c], np.int64)
                    assert (lane_off % 16 == 0).all()
                    for j in range(8):
                        at = slot * half + lane_off // 2 + j
                        if t.feat[ks, h, j] >= 0:
                            pos[:, t.feat[ks, h, j]] = at
                        else:
                            pad.append(at)
            assert (pos >= 0).all()
            self.pos[t.name] = pos
            self.pad[t.name] = np.stack(pad, 1) if pad else np.zeros((self.cols, 0), np.int64)
        for k in masks:  # bit index inside the mask's slot
            pos = np.full((self.cols, k.width), -1, np.int64)
            for ks in range(k.feat.shape[0]):
                for h in range(2):
                    for j in range(8):
                        pos[:, k.feat[ks, h, j]] = (c + self.cols * h) * 16 * 8 + k.bit[ks, j]  # inside the slot
            assert (pos >= 0).all()
            self.mask_pos[k.name] = pos

    def tile_bytes(self):
        return self.n_slots * self.frag_bytes

    def tiles_of(self, nbytes):
        assert nbytes % self.tile_bytes() == 0, f"{nbytes} bytes is not a whole number of {self.tile_bytes()}-byte tiles"
        return nbytes // self.tile_bytes()

    def bit_owners(self):
        """per BIT of a tile's block: how many tensor elements / mask bits live there (0 = zero or pad region)"""
        own = np.zeros(self.tile_bytes() * 8, np.int32)
        for pos in self.pos.values():
            for b in range(16):
                np.add.at(own, pos.reshape(-1) * 16 + b, 1)
        for name, pos in self.mask_pos.items():
            np.add.at(own, self.masks[name].slot * self.frag_bytes * 8 + pos.reshape(-1), 1)
        return own

    # -- decoding / encoding of whole buffers --
    def _blocks(self, buf_u8):
        b = buf_u8.detach().cpu().numpy() if isinstance(buf_u8, torch.Tensor) else np.asarray(buf_u8)
        assert b.dtype == np.uint8 and b.ndim == 1
        n_tiles = self.tiles_of(b.size)
        return np.ascontiguousarray(b).reshape(n_tiles, self.tile_bytes()), n_tiles

    def read(self, blocks, name):
        """-> float64 [tiles * 32, width], uint16 raw pad k-slots [tiles * 32, n_pad]"""
        u16 = blocks.view(np.uint16)
        val = bf16_bits_to_f64(u16[:, self.pos[name].reshape(-1)]).reshape(-1, self.tensors[name].width)
        pad = u16[:, self.pad[name].reshape(-1)].reshape(val.shape[0], -1)
        return val, pad

    def _mask_slot(self, blocks, name):
        s = self.masks[name].slot
        return blocks[:, s * self.frag_bytes:(s + 1) * self.frag_bytes]

    def read_mask(self, blocks, name):
        bits = np.unpackbits(self._mask_slot(blocks, name), axis=1, bitorder="little")
        return bits[:, self.mask_pos[name].reshape(-1)].reshape(-1, self.masks[name].width).astype(bool)

    def write(self, blocks, name, val):
        u16 = blocks.view(np.uint16)
        u16[:, self.pos[name].reshape(-1)] = f64_to_bf16_bits(val).reshape(blocks.shape[0], -1)

    def write_mask(self, blocks, name, val):
        slot = self._mask_slot(blocks, name)
        bits = np.unpackbits(slot, axis=1, bitorder="little")
        bits[:, self.mask_pos[name].reshape(-1)] = np.asarray(val, np.uint8).reshape(blocks.shape[0], -1)
        slot[:] = np.packbits(bits, axis=1, bitorder="little")


def load_host_lib():
    if not os.path.exists(HOST_LIB):
        raise FileNotFoundError(f"{HOST_LIB} not built (run __graft_entry__.build())")
    return ctypes.CDLL(HOST_LIB)


def _feat_table(fn, nks):
    return np.array([[[fn(ks, h, j) for j in range(8)] for h in range(2)] for ks in range(nks)], np.int64)


def _stream_feat(lib, t, cols):
    """k-slot -> feature map of the B operand of transposed stream layer t, read off the weights bwd_weight_index() puts
    in A row 0 of its out tile 0: `cols` maps a Dense layer to the first feature its output columns stand for."""
    nk, base = lib.lnrf_host_bwd_layer_info(t, 0), lib.lnrf_host_bwd_layer_info(t, 2)
    offs = dense_offsets()
    feat = np.full((nk, 2, 8), -1, np.int64)
    for ks in range(nk):
        for h in range(2):
            for j in range(8):
                idx = lib.lnrf_host_bwd_weight_index(base + ks, 32 * h, j)
                if idx < 0:
                    continue
                (layer,) = [l for l, (w, b, _, _) in enumerate(offs) if w <= idx < b]
                w, _, _, fo = offs[layer]
                assert (idx - w) // fo == 0 and layer in cols, (t, ks, h, j, idx)
                feat[ks, h, j] = cols[layer] + (idx - w) % fo
    return feat


@functools.lru_cache(maxsize=None)
def layouts():
    """-> (save layout, gradient-dump layout), built once per process from the host layout library"""
    lib = load_host_lib()
    S, G = lib.lnrf_host_save_slot, lib.lnrf_host_grad_slot
    hid = _feat_table(lib.lnrf_host_hidden_feat, 16)
    save_t = [TensorMap("x_emb", S(0, 0), _feat_table(lib.lnrf_host_xemb_feat, 4), X_EMB)]
    save_t += [TensorMap(f"h{l}", S(1, l), hid, HIDDEN) for l in range(8)]
    save_t += [TensorMap("z", S(2, 0), hid, HIDDEN), TensorMap("d_emb", S(3, 0), _feat_table(lib.lnrf_host_demb_feat, 2), D_EMB),
               TensorMap("h10", S(4, 0), hid[:COLOR // 16], COLOR)]
    bit = np.array([[lib.lnrf_host_mask_bit(ks, j) for j in range(8)] for ks in range(16)])
    save_m = [MaskMap(f"mask{l}", S(5, 0) + l, hid, bit, HIDDEN) for l in range(8)]
    save_m += [MaskMap("mask10", S(5, 0) + 8, hid[:COLOR // 16], bit[:COLOR // 16], COLOR)]
    save = DumpLayout(lib, S(6, 0), save_t, save_m)
    grad_t = [TensorMap("dy11", G(0, 0), _stream_feat(lib, 0, {11: 0}), 3),
              TensorMap("dy10m", G(1, 0), _stream_feat(lib, 1, {10: 0, 9: COLOR}), COLOR + 1)]  # feature 128 = density logit
    grad_t += [TensorMap(f"dy{l}", G(2, l), hid, HIDDEN) for l in range(9)]
    grad = DumpLayout(lib, G(3, 0), grad_t, [])
    return save, grad


def _zero_slots(lay, blocks):
    """raw bytes [tiles, 1 KiB] of every slot no tensor or mask lives in"""
    used = {t.slot0 + ks for t in lay.tensors.values() for ks in range(t.nks)} | {k.slot for k in lay.masks.values()}
    fb = lay.frag_bytes
    return {s: blocks[:, s * fb:(s + 1) * fb].copy() for s in range(lay.n_slots) if s not in used}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def decode_save(buf_u8, m, hidden_masks=True):
    """Forward save -> float64 / bool CPU tensors in Flax feature order, rows = evaluations 0..m-1:
    x_emb[m,60], h[l][m,256] (l = 0..7), z[m,256], d_emb[m,24], h10[m,128], mask[l][m,256] (None where the slots were not
    written: hidden_masks=False, the save of lnrf_nerf_mlp_fwd_ls), mask10[m,128];
    "pad": the same tensors for the pad evaluations m .. 32 * tiles of the buffer; "pad_slots": the raw uint16 of the unused
    k-slots of x_emb and d_emb (all rows); "mask10_high": the 8 bytes per lane of the h10 mask slot that carry no bit."""
    lay, _ = layouts()
    blocks, n_tiles = lay._blocks(buf_u8)
    assert 0 < m <= n_tiles * lay.cols
    out, pad, pad_slots = {}, {}, {}
    for name in lay.tensors:
        val, ps = lay.read(blocks, name)
        out[name], pad[name] = _t(val[:m]), _t(val[m:])
        if ps.shape[1]:
            pad_slots[name] = _t(ps.astype(np.int32))
    for name in lay.masks:
        if name == "mask10" or hidden_masks:
            val = lay.read_mask(blocks, name)
            out[name], pad[name] = _t(val[:m]), _t(val[m:])
        else:
            out[name] = None
    res = {k: out[k] for k in ("x_emb", "z", "d_emb", "h10", "mask10")}
    res["h"] = [out[f"h{l}"] for l in range(8)]
    res["mask"] = [out[f"mask{l}"] for l in range(8)]
    res["pad"], res["pad_slots"] = pad, pad_slots
    k10 = lay.masks["mask10"]
    lanes = blocks[:, k10.slot * lay.frag_bytes:(k10.slot + 1) * lay.frag_bytes].reshape(n_tiles, -1, 16)
    res["mask10_high"] = _t(lanes[:, :, k10.width // 16:].copy())
    return res


def decode_grad(buf_u8, m):
    """Gradient dump -> dy[l][m,256] (l = 0..8), dy10[m,128], dlogit[m], dy11[m,3] as float64 CPU tensors; "pad": dy11,
    dy10m, dy0..8 of the pad evaluations; "pad_slots": raw uint16 of the unused k-slots of dy11 and dy10m (all rows);
    "zero_slots": {slot: raw bytes [tiles, 1024]} of the slots that hold no tensor.  Trailing bytes of `buf_u8` behind the
    dump (the slabs of the scratch) must be cut off by the caller: pass buf[:grad_dump_bytes(m)]."""
    _, lay = layouts()
    blocks, n_tiles = lay._blocks(buf_u8)
    assert 0 < m <= n_tiles * lay.cols
    vals, pad, pad_slots = {}, {}, {}
    for name in lay.tensors:
        val, ps = lay.read(blocks, name)
        vals[name], pad[name] = val[:m], _t(val[m:])
        if ps.shape[1]:
            pad_slots[name] = _t(ps.astype(np.int32))
    return {"dy": [_t(vals[f"dy{l}"]) for l in range(9)], "dy10": _t(vals["dy10m"][:, :COLOR]),
            "dlogit": _t(vals["dy10m"][:, COLOR]), "dy11": _t(vals["dy11"]), "pad": pad, "pad_slots": pad_slots,
            "zero_slots": {s: _t(v) for s, v in _zero_slots(lay, blocks).items()}}


def grad_dump_bytes(m):
    """bytes of the gradient dump at the front of a backward scratch for m evaluations"""
    _, lay = layouts()
    return padded_tiles(m) * lay.tile_bytes()


def padded_tiles(m):
    lib = load_host_lib()
    cols, group = lib.lnrf_host_dump_info(1), lib.lnrf_host_dump_info(2)
    return (-(-m // cols) + group - 1) // group * group


def _rows(val, n_rows, width):
    full = np.zeros((n_rows, width), np.float64)
    v = np.asarray(val, dtype=np.float64).reshape(-1, width)
    full[:v.shape[0]] = v
    return full


def encode_save(t, m, hidden_masks=True):
    """inverse of decode_save for tensors of m rows (pad evaluations, pad k-slots and unwritten masks stay zero)"""
    lay, _ = layouts()
    n_tiles = padded_tiles(m)
    blocks = np.zeros((n_tiles, lay.tile_bytes()), np.uint8)
    named = {"x_emb": t["x_emb"], "z": t["z"], "d_emb": t["d_emb"], "h10": t["h10"]}
    named.update({f"h{l}": t["h"][l] for l in range(8)})
    for name, val in named.items():
        lay.write(blocks, name, _rows(val, n_tiles * lay.cols, lay.tensors[name].width))
    masks = {"mask10": t["mask10"]}
    if hidden_masks:
        masks.update({f"mask{l}": t["mask"][l] for l in range(8)})
    for name, val in masks.items():
        lay.write_mask(blocks, name, _rows(val, n_tiles * lay.cols, lay.masks[name].width) != 0)
    return blocks.reshape(-1)


def encode_grad(t, m):
    _, lay = layouts()
    n_tiles = padded_tiles(m)
    blocks = np.zeros((n_tiles, lay.tile_bytes()), np.uint8)
    dy10m = np.concatenate([np.asarray(t["dy10"], np.float64), np.asarray(t["dlogit"], np.float64).reshape(-1, 1)], 1)
    named = {"dy11": t["dy11"], "dy10m": dy10m}
    named.update({f"dy{l}": t["dy"][l] for l in range(9)})
    for name, val in named.items():
        lay.write(blocks, name, _rows(val, n_tiles * lay.cols, lay.tensors[name].width))
    return blocks.reshape(-1)


# ---- Ref-NeRF directional block -----------------------------------------------------------------------------------------
def _dir_dy10_feat(lib, n_slots):
    """k-slot -> colour channel map of dy10, read off the Dense_10^T rows of the transposed directional stream (as
    _stream_feat does for dy11): k-slot (h, j) of its one k-step carries the channel whose weight of hidden feature 0 the
    pack walk puts in A row 0 of out tile 0.  The slots behind the first carry nothing."""
    lib.lnrf_host_stream_indices.restype = ctypes.c_int64
    lib.lnrf_host_stream_indices.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    n = lib.lnrf_host_stream_indices(6, 0, None)
    idx = np.empty(n, np.int32)
    assert lib.lnrf_host_stream_indices(6, 0, idx.ctypes.data) == n
    idx = idx.reshape(-1, 64, 8)
    w10, b10 = lib.lnrf_host_wgrad_const(6), lib.lnrf_host_wgrad_const(7)
    feat = np.full((n_slots, 2, 8), -1, np.int64)
    for h in range(2):
        for j in range(8):
            i = int(idx[0, lib.lnrf_host_dump_info(1) * h, j])
            if i >= 0:
                assert w10 <= i < b10 and (i - w10) // 3 == 0, (h, j, i)
                feat[0, h, j] = (i - w10) % 3
    return feat


@functools.lru_cache(maxsize=None)
def dir_layouts():
    """-> (directional save layout, directional gradient-dump layout), from the host layout library"""
    lib = load_host_lib()
    S = lib.lnrf_host_dir_slot
    nks_in, nks_h = -(-DIR_IN // 16), DIR_HIDDEN // 16
    assert S(1) - S(0) == nks_in and S(2) - S(1) == nks_h and S(6) - S(5) == nks_h
    hid = _feat_table(lib.lnrf_host_hidden_feat, nks_in)
    bit = np.array([[lib.lnrf_host_mask_bit(ks, j) for j in range(8)] for ks in range(nks_h)])
    save = DumpLayout(lib, S(3), [TensorMap("xin", S(0), np.where(hid < DIR_IN, hid, -1), DIR_IN),
                                  TensorMap("h9", S(1), hid[:nks_h], DIR_HIDDEN)],
                      [MaskMap("mask9", S(2), hid[:nks_h], bit, DIR_HIDDEN)])
    grad = DumpLayout(lib, S(6), [TensorMap("dy10", S(4), _dir_dy10_feat(lib, S(5) - S(4)), 3),
                                  TensorMap("dy9", S(5), hid[:nks_h], DIR_HIDDEN)], [])
    return save, grad


def _decode(lay, buf_u8, m):
    blocks, n_tiles = lay._blocks(buf_u8)
    assert 0 < m <= n_tiles * lay.cols
    out, pad, pad_slots = {}, {}, {}
    for name in lay.tensors:
        val, ps = lay.read(blocks, name)
        out[name], pad[name] = _t(val[:m]), _t(val[m:])
        if ps.shape[1]:
            pad_slots[name] = _t(ps.astype(np.int32))
    for name in lay.masks:
        val = lay.read_mask(blocks, name)
        out[name], pad[name] = _t(val[:m]), _t(val[m:])
    out["pad"], out["pad_slots"] = pad, pad_slots
    out["zero_slots"] = {s: _t(v) for s, v in _zero_slots(lay, blocks).items()}
    return out, blocks, n_tiles


def decode_dir_save(buf_u8, m):
    """Directional save -> xin[m,273], h9[m,128] (float64), mask9[m,128] (bool); "pad": the same for the pad evaluations;
    "pad_slots": raw uint16 of the k-slots 273..287 of xin (all rows); "mask9_high": the 8 bytes per lane of the mask slot that
    carry no bit"""
    lay, _ = dir_layouts()
    out, blocks, n_tiles = _decode(lay, buf_u8, m)
    k = lay.masks["mask9"]
    lanes = blocks[:, k.slot * lay.frag_bytes:(k.slot + 1) * lay.frag_bytes].reshape(n_tiles, -1, 16)
    out["mask9_high"] = _t(lanes[:, :, k.width // 16:].copy())
    return out


def decode_dir_grad(buf_u8, m):
    """Directional gradient dump -> dy10[m,3], dy9[m,128]; "pad": the pad evaluations; "pad_slots": raw uint16 of the unused
    k-slots of dy10, its whole second slot included (all rows).  Pass buf[:dir_grad_dump_bytes(m)]."""
    return _decode(dir_layouts()[1], buf_u8, m)[0]


def dir_grad_dump_bytes(m):
    return padded_tiles(m) * dir_layouts()[1].tile_bytes()


def _encode(lay, t, m):
    n_tiles = padded_tiles(m)
    blocks = np.zeros((n_tiles, lay.tile_bytes()), np.uint8)
    for name in lay.tensors:
        lay.write(blocks, name, _rows(t[name], n_tiles * lay.cols, lay.tensors[name].width))
    for name in lay.masks:
        lay.write_mask(blocks, name, _rows(t[name], n_tiles * lay.cols, lay.masks[name].width) != 0)
    return blocks.reshape(-1)


def encode_dir_save(t, m):
    """inverse of decode_dir_save for xin, h9, mask9 of m rows (everything else stays zero)"""
    return _encode(dir_layouts()[0], t, m)


def encode_dir_grad(t, m):
    return _encode(dir_layouts()[1], t, m)


# ---- the two comparison rules -----------------------------------------------------------------------------------------
def dot_delta(k, abs_sum):
    """admissible error of an fp32-accumulated dot product of exact bf16 x bf16 products: (K + 2) 2^-23 sum |a||b| (+ |bias|),
    K = contraction length including the pad k-steps"""
    return (k + 2) * U23 * np.asarray(abs_sum, dtype=np.float64)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def check_rounded(got_bf16, ref_f64, delta, relu=False, what=""):
    """The rule for every tensor the kernels round to bf16.  `got_bf16`: the decoded bf16 values; `ref_f64`: the float64
    value before that rounding (before the ReLU if `relu`); `delta`: the admissible error of the fp32 value that was
    rounded, per element.  got must be bf16_rne(ref) bit for bit (the two zeros count as one value) unless ref lies
    within delta of a rounding boundary — the midpoint between neighbouring bf16 values, and 0 after a ReLU — where either
    side of the boundary passes: got must lie in [bf16_rne(f(ref - delta)), bf16_rne(f(ref + delta))], f = ReLU or identity.
    -> (elements whose interval has two ends = that used the allowance, elements that differ from bf16_rne(f(ref)));
    raises AssertionError naming the worst offenders as (evaluation, feature, got, ref, delta)."""
    got, ref = _np(got_bf16).astype(np.float64), _np(ref_f64).astype(np.float64)
    delta = np.broadcast_to(_np(delta).astype(np.float64), ref.shape)
    assert got.shape == ref.shape and (delta >= 0).all() and np.isfinite(ref).all() and np.isfinite(got).all(), what
    f = (lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v)
    lo, hi, mid = bf16_rne(f(ref - delta)), bf16_rne(f(ref + delta)), bf16_rne(f(ref))
    bad = (got < lo) | (got > hi)
    n_allow, n_diff = int((lo != hi).sum()), int((got != mid).sum())
    if bad.any():
        g2, r2, d2 = (a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(-1, 1) for a in (got, ref, delta))
        ev, ft = np.nonzero(bad.reshape(g2.shape))
        order = np.argsort(-np.abs(g2[ev, ft] - f(r2[ev, ft])))[:8]
        rows = "\n".join(f"    evaluation {ev[i]} feature {ft[i]}: got {float(g2[ev[i], ft[i]])!r} ref {float(r2[ev[i], ft[i]])!r} "
                         f"delta {d2[ev[i], ft[i]]:.3e}" for i in order)
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements are not the bf16 rounding of the reference "
                             f"(allowance region {n_allow}, differing from bf16_rne(ref) {n_diff}); worst:\n{rows}")
    return n_allow, n_diff


def needed_share_of_delta(got_bf16, ref_f64, delta, relu=False):
    """largest part of delta an element needed: distance from ref to the reals that round to got, over delta (reporting)"""
    got, ref = _np(got_bf16).astype(np.float64), _np(ref_f64).astype(np.float64)
    delta = np.broadcast_to(_np(delta).astype(np.float64), ref.shape)
    key = _bf16_key(got)
    lo_edge, hi_edge = (got + _bf16_of_key(key - 1)) / 2, (got + _bf16_of_key(key + 1)) / 2
    if relu:
        lo_edge = np.where(got == 0, -np.inf, lo_edge)
    need = np.maximum(np.maximum(lo_edge - ref, ref - hi_edge), 0.0)
    ok = delta > 0
    return float((need[ok] / delta[ok]).max()) if ok.any() else 0.0


def check_accumulated(got_f32, ref_f64, n_add, abs_sum, what=""):
    """The rule for fp32 results that are never rounded to bf16 (weight and bias gradients): element-wise
    |got - ref| <= (n_add + 2) 2^-23 abs_sum, abs_sum = the same contraction with absolute values.
    -> the largest error-to-bound ratio; raises AssertionError naming the worst offenders."""
    got, ref = _np(got_f32).astype(np.float64), _np(ref_f64).astype(np.float64)
    s = _np(abs_sum).astype(np.float64)
    assert got.shape == ref.shape == s.shape and np.isfinite(got).all(), what
    err, bound = np.abs(got - ref), (n_add + 2) * U23 * s
    bad = err > bound
    if bad.any():
        idx = np.flatnonzero(bad)
        order = idx[np.argsort(-(err.reshape(-1)[idx] / np.maximum(bound.reshape(-1)[idx], 1e-300)))][:8]
        rows = "\n".join(f"    element {tuple(int(v) for v in np.unravel_index(i, got.shape))}: got {float(got.reshape(-1)[i])!r} "
                         f"ref {float(ref.reshape(-1)[i])!r} "
                         f"bound {bound.reshape(-1)[i]:.3e}" for i in order)
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements exceed (n_add + 2) 2^-23 abs_sum "
                             f"(n_add {n_add}); worst:\n{rows}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def check_cap(n_diff, n, cpu_flip_share, what=""):
    """The condition that keeps the allowance from hiding a failure: the share of elements that differ from bf16_rne(ref)
    may be at most 10 x the share of the CPU fp32 result of the same operands that does, plus 8 elements."""
    assert n_diff <= 10 * cpu_flip_share * n + 8, (
        f"{what}: {n_diff} of {n} elements differ from bf16_rne(ref) (share {n_diff / n:.3e}); the CPU fp32 result of the "
        f"same operands differs in a share of {cpu_flip_share:.3e}; cap 10 x that + 8 elements")
