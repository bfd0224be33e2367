"""
Mesh comparison (scripts/eval_mesh.py): how far is one triangle mesh from another.  Both surfaces are sampled in
proportion to area (TriangleMesh.sample_surface), every sample is taken to the other mesh by the exact nearest-triangle
query (TriangleMesh.nearest: point to TRIANGLE, so the other side's sampling adds no noise), and the distances are
summed in fp64 in a fixed order (lnrf_dist_stats_f64): two runs with one seed give the same digits.  Definitions, with
P the samples of the predicted mesh, R those of the reference, d(x, M) the pinned distance of csrc/raycast.hip:

  accuracy      mean over P of d(x, ref)            completeness   mean over R of d(x, pred)
  chamfer       accuracy + completeness             chamfer_l2     mean over P of d^2 + mean over R of d^2
  precision(t)  share of P with d <= t              recall(t)      share of R with d <= t
  f_score(t)    2 precision recall / (precision + recall), 0 when both are 0
  hausdorff     max over P and R of d (over the samples: a lower bound of the true Hausdorff distance)
  normal_consistency   the mean of the two directions' means of |n_own . n_nearest|, n the unit face normals in
                float64 (n = e1 x e2 / |e1 x e2|, one torch call per operation, the dot product rounded to fp32);
                samples whose nearest triangle has zero area are left out and counted in normals_skipped.

No alignment is estimated and nothing is culled by visibility.  read_mesh reads .stl, .obj and .ply into triangles.
"""
import ctypes
import math
import struct
from dataclasses import dataclass
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from learn_nerf import _lib as L
from learn_nerf.raycast import TriangleMesh, read_stl

MAX_THRESHOLDS = 8
PRED_STREAM, REF_STREAM = 0, 1  # Philox streams of the two sample sets


# -------------------------------------------------------------- readers ----

def read_mesh(path: str) -> np.ndarray:
    """Triangles [n, 3, 3] float32 of a .stl (read_stl), .obj or .ply file, chosen by extension.  ValueError naming the
    file for anything malformed, for a mesh without faces and for non-finite vertices."""
    ext = path.lower().rsplit(".", 1)[-1] if "." in path else ""
    if ext == "stl":
        return read_stl(path)
    if ext == "obj":
        verts, faces = _read_obj(path)
    elif ext == "ply":
        verts, _, faces = read_ply(path)
    else:
        raise ValueError(f"{path}: unknown mesh format: expected a .stl, .obj or .ply file")
    if len(faces) == 0:
        raise ValueError(f"{path}: the mesh holds no triangles")
    if faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError(f"{path}: a face names vertex {int(faces.max() if faces.max() >= len(verts) else faces.min())}"
                         f", the file has {len(verts)}")
    if not np.isfinite(verts).all():
        raise ValueError(f"{path}: the mesh holds non-finite vertices")
    return np.ascontiguousarray(verts[faces], dtype=np.float32)


def _fan(indices):
    return [(indices[0], indices[k], indices[k + 1]) for k in range(1, len(indices) - 1)]


def _read_obj(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """'v x y z [more]' (trailing colours or w are ignored) and 'f' with a, a/b, a/b/c, a//c entries, 1-based or
    negative (relative to the vertices read so far); polygons are fan-triangulated.  Other records are ignored."""
    verts, faces = [], []
    try:
        with open(path, "r", encoding="utf-8", errors="strict") as handle:
            lines = handle.read().splitlines()
    except UnicodeDecodeError:
        raise ValueError(f"{path}: malformed OBJ: not text") from None
    for number, line in enumerate(lines, 1):
        parts = line.split("#", 1)[0].split()
        if not parts:
            continue
        if parts[0] == "v":
            try:
                verts.append([float(parts[1]), float(parts[2]), float(parts[3])])
            except (IndexError, ValueError):
                raise ValueError(f"{path}: malformed OBJ: line {number}: a 'v' without three numbers") from None
        elif parts[0] == "f":
            if len(parts) < 4:
                raise ValueError(f"{path}: malformed OBJ: line {number}: a face of fewer than 3 vertices")
            corner = []
            for entry in parts[1:]:
                try:
                    index = int(entry.split("/")[0])
                except ValueError:
                    raise ValueError(f"{path}: malformed OBJ: line {number}: bad face entry {entry!r}") from None
                if index == 0 or index > len(verts) or index < -len(verts):
                    raise ValueError(f"{path}: malformed OBJ: line {number}: face entry {entry!r} names no vertex read "
                                     f"so far ({len(verts)})")
                corner.append(index - 1 if index > 0 else len(verts) + index)
            faces.extend(_fan(corner))
    return (np.asarray(verts, dtype=np.float64).reshape(-1, 3).astype(np.float32),
            np.asarray(faces, dtype=np.int64).reshape(-1, 3))


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path: str):
    """(verts float32 [V, 3], colours uint8 [V, 3] or None, faces int64 [F, 3]) of an ASCII or binary little-endian
    PLY: vertex properties in any order (x, y, z required; red, green, blue kept when all are there), faces as a list
    property named vertex_indices or vertex_index, polygons fan-triangulated; other elements are skipped."""
    with open(path, "rb") as handle:
        data = handle.read()
    if not data.startswith(b"ply"):
        raise ValueError(f"{path}: malformed PLY: the file does not start with 'ply'")
    end = data.find(b"end_header")
    newline = data.find(b"\n", end) if end >= 0 else -1
    if end < 0 or newline < 0:
        raise ValueError(f"{path}: truncated PLY: the header has no 'end_header'")
    try:
        header = data[:end].decode("ascii").splitlines()
    except UnicodeDecodeError:
        raise ValueError(f"{path}: malformed PLY: the header is not ASCII") from None
    body = newline + 1
    fmt, elements = None, []
    try:
        for line in header[1:]:
            words = line.split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words[0] == "format":
                fmt = words[1]
            elif words[0] == "element":
                elements.append((words[1], int(words[2]), []))
            elif words[0] == "property":
                if not elements:
                    raise ValueError
                if words[1] == "list":
                    elements[-1][2].append((words[4], _PLY_TYPES[words[2]], _PLY_TYPES[words[3]]))
                else:
                    elements[-1][2].append((words[2], _PLY_TYPES[words[1]], None))
            else:
                raise ValueError
    except (IndexError, ValueError, KeyError):
        raise ValueError(f"{path}: malformed PLY: header line {line!r}") from None
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unsupported PLY format {fmt!r}: expected ascii or binary_little_endian")
    if any(count < 0 for _, count, _ in elements):
        raise ValueError(f"{path}: malformed PLY: a negative element count")
    tokens = data[body:].split() if fmt == "ascii" else None
    pos = 0 if fmt == "ascii" else body
    verts, colors, faces = None, None, np.zeros((0, 3), np.int64)
    try:
        for name, count, props in elements:
            scalar_only = all(item is None for _, _, item in props)
            if scalar_only:
                if fmt == "ascii":
                    width = len(props)
                    if pos + count * width > len(tokens):
                        raise IndexError
                    table = np.array([float(t) for t in tokens[pos:pos + count * width]], np.float64)
                    table = table.reshape(count, width)
                    pos += count * width
                    columns = {p[0]: table[:, k].astype(p[1]) for k, p in enumerate(props)}
                else:
                    dtype = np.dtype([(f"f{k}", "<" + p[1]) for k, p in enumerate(props)])
                    if pos + count * dtype.itemsize > len(data):
                        raise IndexError
                    rec = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
                    pos += count * dtype.itemsize
                    columns = {p[0]: rec[f"f{k}"] for k, p in enumerate(props)}
                if name == "vertex":
                    if not all(axis in columns for axis in "xyz"):
                        raise ValueError(f"{path}: malformed PLY: the vertex element lacks x, y or z")
                    verts = np.stack([columns[axis] for axis in "xyz"], axis=1).astype(np.float32)
                    if all(c in columns for c in ("red", "green", "blue")):
                        colors = np.stack([columns[c] for c in ("red", "green", "blue")], axis=1).astype(np.uint8)
                continue
            if (fmt != "ascii" and name == "face" and len(props) == 1
                    and props[0][0] in ("vertex_indices", "vertex_index")):
                # all triangles (what every writer here produces): one structured read instead of a row loop
                dtype = np.dtype([("n", "<" + props[0][1]), ("idx", "<" + props[0][2], (3,))])
                if pos + count * dtype.itemsize <= len(data):
                    rec = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
                    if (rec["n"] == 3).all():
                        faces = rec["idx"].astype(np.int64).reshape(-1, 3)
                        pos += count * dtype.itemsize
                        continue
            rows = []
            for _ in range(count):
                row = {}
                for pname, ptype, item in props:
                    if fmt == "ascii":
                        if item is None:
                            row[pname] = float(tokens[pos])
                            pos += 1
                        else:
                            k = int(tokens[pos])
                            if k < 0 or pos + 1 + k > len(tokens):
                                raise IndexError
                            row[pname] = [int(t) for t in tokens[pos + 1:pos + 1 + k]]
                            pos += 1 + k
                    else:
                        if item is None:
                            pos += np.dtype(ptype).itemsize
                            if pos > len(data):
                                raise IndexError
                        else:
                            (k,) = struct.unpack_from("<" + np.dtype(ptype).char, data, pos)
                            pos += np.dtype(ptype).itemsize
                            size = np.dtype(item).itemsize
                            if k < 0 or pos + k * size > len(data):
                                raise IndexError
                            row[pname] = np.frombuffer(data, dtype="<" + item, count=k, offset=pos).tolist()
                            pos += k * size
                rows.append(row)
            if name == "face":
                key = next((p[0] for p in props if p[0] in ("vertex_indices", "vertex_index")), None)
                if key is None:
                    raise ValueError(f"{path}: malformed PLY: the face element has no vertex_indices list")
                tris = []
                for row in rows:
                    if len(row[key]) < 3:
                        raise ValueError(f"{path}: malformed PLY: a face of fewer than 3 vertices")
                    tris.extend(_fan(row[key]))
                faces = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    except (IndexError, struct.error):
        raise ValueError(f"{path}: truncated PLY: the data ends before the elements the header counts") from None
    except ValueError as err:
        if str(err).startswith(path):
            raise
        raise ValueError(f"{path}: malformed PLY: {err}") from None
    if verts is None:
        raise ValueError(f"{path}: malformed PLY: no vertex element")
    return verts, colors, faces


# -------------------------------------------------------------- metrics ----

@dataclass
class MeshComparison:
    accuracy: float
    completeness: float
    chamfer: float
    chamfer_l2: float
    thresholds: Tuple[float, ...]
    precision: Tuple[float, ...]
    recall: Tuple[float, ...]
    f_score: Tuple[float, ...]
    hausdorff: float
    normal_consistency: float
    samples: int
    normals_skipped: int  # samples whose nearest triangle has zero area, both directions
    degenerate_triangles: Tuple[int, int]  # zero-area triangles of pred and ref: never sampled
    per_sample: Dict[str, torch.Tensor]  # {pred,ref}_{points,distance,ids,nearest}: GPU tensors, one row per sample


def unit_normals(tris: torch.Tensor, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(n float64 [m, 3], length float64 [m]) of the triangles tris[ids]: n = e1 x e2 / length, 0 where length is 0;
    one torch call per operation, length = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z)."""
    v = tris[ids.long()].double()
    e1 = [v[:, 1, a] - v[:, 0, a] for a in range(3)]
    e2 = [v[:, 2, a] - v[:, 0, a] for a in range(3)]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    length = torch.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    zero = torch.zeros_like(length)
    return torch.stack([torch.where(length > 0, c / length, zero) for c in n], dim=1), length


def normal_cosines(own: TriangleMesh, own_ids: torch.Tensor, other: TriangleMesh,
                   near_ids: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(cosine fp32 [m], skipped): n_own . n_nearest per sample, 0 where the nearest triangle has zero area."""
    a, _ = unit_normals(own.tris, own_ids)
    b, length = unit_normals(other.tris, near_ids)
    cosine = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    return cosine.to(torch.float32).contiguous(), int((length == 0).sum().item())


def dist_stats_(d2: torch.Tensor, cosine, thresholds: Sequence[float], acc: torch.Tensor) -> torch.Tensor:
    """acc (float64 [4 + K], GPU) += the statistics of lnrf_dist_stats_f64 over d2 fp32 [m] (and cosine fp32 [m])."""
    k = len(thresholds)
    if k > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds, got {k}")
    if d2.dim() != 1 or (cosine is not None and cosine.shape != d2.shape):
        raise ValueError("dist_stats_: d2 and cosine must be [m]")
    if acc.dtype != torch.float64 or tuple(acc.shape) != (4 + k,):
        raise ValueError(f"dist_stats_: acc must be float64 of shape [{4 + k}]")
    m = d2.shape[0]
    if m == 0:
        return acc
    nbytes = L.lib().lnrf_dist_stats_scratch_bytes(m)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=d2.device)
    taus = (ctypes.c_double * max(k, 1))(*[float(t) for t in thresholds])
    L.check(L.lib().lnrf_dist_stats_f64(L.ptr(d2), L.ptr(cosine), m, taus, k, L.ptr(acc, torch.float64),
                                        L.ptr(scratch, torch.float64), nbytes, L.stream()), "dist_stats_f64")
    return acc


def metrics_from_stats(pred_acc, ref_acc, samples: int, pred_valid: int, ref_valid: int, thresholds):
    """The metric definitions of the module docstring from the two accumulators of lnrf_dist_stats_f64 (sequences of
    4 + K floats): plain Python float arithmetic, so that a restatement reproduces every digit."""
    m = float(samples)
    accuracy, completeness = pred_acc[0] / m, ref_acc[0] / m
    precision = tuple(pred_acc[4 + k] / m for k in range(len(thresholds)))
    recall = tuple(ref_acc[4 + k] / m for k in range(len(thresholds)))
    f_score = tuple(2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall))
    means = [acc[2] / valid for acc, valid in ((pred_acc, pred_valid), (ref_acc, ref_valid)) if valid > 0]
    return dict(accuracy=accuracy, completeness=completeness, chamfer=accuracy + completeness,
                chamfer_l2=pred_acc[1] / m + ref_acc[1] / m, precision=precision, recall=recall, f_score=f_score,
                hausdorff=math.sqrt(max(pred_acc[3], ref_acc[3])),
                normal_consistency=sum(means) / len(means) if means else math.nan)


def compare_meshes(pred_tris, ref_tris, samples: int = 1_000_000, thresholds: Sequence[float] = (0.01,),
                   seed: int = 0, device=None) -> MeshComparison:
    """The metrics of the module docstring between two triangle sets [n, 3, 3] (arrays or tensors), from `samples`
    surface samples per side.  The pinned queries run on the GPU; there is no CPU fallback."""
    thresholds = tuple(float(t) for t in thresholds)
    if not 1 <= len(thresholds) <= MAX_THRESHOLDS:
        raise ValueError(f"between 1 and {MAX_THRESHOLDS} thresholds, got {len(thresholds)}")
    if not all(t >= 0 and math.isfinite(t) for t in thresholds):
        raise ValueError("thresholds must be finite and not negative")
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"samples must be positive, got {samples}")
    device = torch.device("cuda" if device is None else device)

    def as_mesh(tris):
        if not isinstance(tris, torch.Tensor):
            tris = torch.from_numpy(np.ascontiguousarray(np.asarray(tris, dtype=np.float32)))
            tris = tris.to(device)
        return TriangleMesh(tris)

    pred, ref = as_mesh(pred_tris), as_mesh(ref_tris)
    out, accs, valid, skipped, degenerate = {}, [], [], 0, []
    for name, own, other, stream in (("pred", pred, ref, PRED_STREAM), ("ref", ref, pred, REF_STREAM)):
        degenerate.append(int((own.tri_areas() == 0).sum().item()))
        points, own_ids = own.sample_surface(samples, seed, stream_id=stream)
        d2, near_ids = other.nearest(points)
        cosine, bad = normal_cosines(own, own_ids, other, near_ids)
        acc = torch.zeros(4 + len(thresholds), dtype=torch.float64, device=points.device)
        dist_stats_(d2, cosine, thresholds, acc)
        accs.append(acc.tolist())
        valid.append(samples - bad)
        skipped += bad
        out[name + "_points"], out[name + "_distance"] = points, d2.double().sqrt().to(torch.float32)
        out[name + "_ids"], out[name + "_nearest"] = own_ids, near_ids
    values = metrics_from_stats(accs[0], accs[1], samples, valid[0], valid[1], thresholds)
    return MeshComparison(thresholds=thresholds, samples=samples, normals_skipped=skipped,
                          degenerate_triangles=(degenerate[0], degenerate[1]), per_sample=out, **values)
