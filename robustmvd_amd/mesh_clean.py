"""Mesh clean-up: the connected components of a triangle mesh, their table, the removal of small components ("floaters") and
area-weighted vertex normals.  It is the last step of the reconstruction chain (depth maps -> DepthFusion -> TSDFVolume -> Mesh): a
TSDF fused from real depth carries small closed blobs wherever a few views agreed on a wrong depth.  The reference has no such
component; the definition is this docstring, the *_numpy functions (the readable specification and the CPU path) and include/mvd.h.

Inputs.  vertices (M,3) float32, triangles (T,3) integers in 0 .. M-1 (int32 on a GPU).  Two vertices are connected when a triangle
names both; degenerate (i,i,j) and duplicate triangles connect like any other.  Coordinates play no part in the connectivity.

  1. Labels.  label[v] = the lowest vertex index of v's component: a unique fixed point.  components_numpy and the kernels reach it
     by rounds of min-label hooking with pointer jumping (FastSV): per triangle (a,b,c), m = min over x of label[label[x]] lowers
     label[label[x]] and label[x]; then label[v] = label[label[v]] per vertex; until a round changes nothing.  The number of rounds
     is at most max_rounds(M) = 2 ceil(log2(max(M,2))) + 4, or RuntimeError: shuffled quad strips, the long-diameter case, take
     8, 10 and 14 rounds at M = 1026, 16386 and 262146 (the kernels 7, 8 and 10), the unchanged last one included.  A vertex no
     triangle names is UNREFERENCED: it is its own label and belongs to no component.
  2. Components.  Ids 0 .. C-1 in ascending order of the components' lowest vertex.  vertex_component (M): the id, -1 for an
     unreferenced vertex.  triangle_component (T): the id of the triangle's first vertex.  num_triangles, num_vertices (C).
  3. Area.  Of a triangle: e1 = p1 - p0, e2 = p2 - p0 in float64 from the float32 coordinates, n = (e1y e2z - e1z e2y,
     e1z e2x - e1x e2z, e1x e2y - e1y e2x), area = 0.5 sqrt((nx nx + ny ny) + nz nz), one rounding per operation; 0 where that is not
     finite.  Of a component: the float64 sum of its triangles' areas in ascending triangle index.  (The device adds a component of
     more than 64 triangles as interleaved partial sums in a fixed tree, include/mvd.h: the same value within the rounding of n
     float64 additions, and the same bits in every run.)
  4. Filter.  A component stays when it passes ALL given criteria: min_triangles (num_triangles >= it), min_area (area >= it),
     keep_largest=k (among the k components with the most triangles, ties to the lower id).  With no criterion every triangle
     stays.  Kept triangles keep their order; kept vertices keep theirs; remove_unreferenced (the default) drops every vertex no
     kept triangle names; triangles are re-indexed; colours, normals and any per-vertex (M,k) float32 array follow bit for bit.
     vertex_remap (M): the new index or -1; kept_triangles: the old index of each kept triangle.
  5. Vertex normals.  The sum over the triangles that name the vertex, once per corner, in ascending (triangle, corner) order, of
     the triangle's un-normalised n of step 3 (area-weighted), in float64; divided by sqrt((sx sx + sy sy) + sz sz) and rounded to
     float32; (0,0,0) where that length is zero or not finite, or the vertex is unreferenced.

Two implementations: the numpy forms on the host and the HIP kernels of csrc/mesh_clean.hip (ops.mesh_*) for a mesh on a GPU, with the
two stable sorts (triangles by component, corners by vertex) through torch.  The public functions pick by where the arrays live.
"""
from dataclasses import dataclass

import numpy as np

from .mesh import Mesh, check_mesh, check_triangles, int32_triangles, is_mesh, one_place, split_mesh, to_numpy


def max_rounds(M):
    """The hard cap of the labelling's rounds, the last (unchanged) one included."""
    return 2 * int(np.ceil(np.log2(max(int(M), 2)))) + 4


@dataclass
class MeshComponents:
    """vertex_component (M) int32, -1: unreferenced; triangle_component (T) int32; per component num_triangles, num_vertices (C) int32
    and area (C) float64; rounds: the labelling's rounds, the unchanged last one included.  numpy arrays or GPU tensors."""
    vertex_component: object
    triangle_component: object
    num_triangles: object
    num_vertices: object
    area: object
    rounds: int

    @property
    def num_components(self):
        return int(self.num_triangles.shape[0])


@dataclass
class CleanResult:
    """clean_mesh's full result: the new mesh, the per-vertex attributes handed in (same container), vertex_remap (M) int32 (new
    index or -1) and kept_triangles (T') int32 (old indices)."""
    mesh: object
    attributes: object
    vertex_remap: object
    kept_triangles: object


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def _check_criteria(min_triangles, min_area, keep_largest):
    if min_triangles is not None and (int(min_triangles) != min_triangles or min_triangles < 0):
        raise ValueError(f"min_triangles must be a non-negative integer, got {min_triangles}")
    if min_area is not None and not float(min_area) >= 0:
        raise ValueError(f"min_area must be a non-negative number, got {min_area}")
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 0):
        raise ValueError(f"keep_largest must be a non-negative integer, got {keep_largest}")
    return not (min_triangles is None and min_area is None and keep_largest is None)


# ---- the numpy forms ------------------------------------------------------------------------------------------------------------------
def components_numpy(triangles, M, details=False):
    """Step 1 -> label (M) int32, the lowest vertex index of each vertex's component (an unreferenced vertex: itself).  The
    synchronous form of the rounds: every hook of a round reads the labels the round started with, the shortcut reads the hooked
    ones.  details=True -> (label, referenced (M) bool, rounds)."""
    M = int(M)
    tri = np.asarray(to_numpy(triangles))
    T = check_triangles(tri, M)
    tri = tri.astype(np.int64)
    label = np.arange(M, dtype=np.int64)
    referenced = np.zeros(M, dtype=bool)
    referenced[tri.ravel()] = True
    rounds = 0
    for rounds in range(1, max_rounds(M) + 1):
        if T == 0:
            break
        grand = label[label]
        m = grand[tri].min(axis=1)
        hooked = label.copy()
        for k in range(3):
            np.minimum.at(hooked, label[tri[:, k]], m)
            np.minimum.at(hooked, tri[:, k], m)
        new = hooked[hooked]
        changed = not np.array_equal(new, label)
        label = new
        if not changed:
            break
    else:
        raise RuntimeError(f"the labelling did not converge within {max_rounds(M)} rounds")
    label = label.astype(np.int32)
    return (label, referenced, rounds) if details else label


def cross_numpy(vertices, triangles):
    """The un-normalised cross products n (T,3) of step 3, float64 from the float32 coordinates."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    t = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    p0 = v[t[:, 0]]
    a, b = v[t[:, 1]] - p0, v[t[:, 2]] - p0
    with np.errstate(all="ignore"):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                        axis=1)


def _length(n):
    with np.errstate(all="ignore"):
        return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def triangle_areas_numpy(vertices, triangles):
    """(T) float64: step 3's area of every triangle, 0 where not finite."""
    area = 0.5 * _length(cross_numpy(vertices, triangles))
    return np.where(np.isfinite(area), area, 0.0)


def component_table_numpy(vertices, triangles):
    """Steps 1 to 3 -> MeshComponents of numpy arrays."""
    vertices, tri = np.asarray(to_numpy(vertices)), np.asarray(to_numpy(triangles))
    M, T = check_mesh(vertices, tri)
    label, referenced, rounds = components_numpy(tri, M, details=True)
    roots = np.nonzero(referenced & (label == np.arange(M)))[0]  # ascending: the ids
    C = len(roots)
    rank = np.full(M, -1, dtype=np.int32)
    rank[roots] = np.arange(C, dtype=np.int32)
    vcomp = np.where(referenced, rank[label], -1).astype(np.int32)
    tcomp = vcomp[tri[:, 0].astype(np.int64)] if T else np.zeros(0, dtype=np.int32)
    # bincount adds its weights one after the other in the order of the list: ascending triangle index within every component
    area = np.bincount(tcomp, weights=triangle_areas_numpy(vertices, tri), minlength=C).astype(np.float64) if T else np.zeros(0)
    return MeshComponents(vcomp, tcomp.astype(np.int32), np.bincount(tcomp, minlength=C).astype(np.int32),
                          np.bincount(vcomp[vcomp >= 0], minlength=C).astype(np.int32), area, rounds)


def keep_components(num_triangles, area, min_triangles=None, min_area=None, keep_largest=None):
    """Step 4's verdict per component -> (C) bool, from the table's counts and areas (numpy, on the host)."""
    nt, area = np.asarray(num_triangles).astype(np.int64), np.asarray(area, dtype=np.float64)
    keep = np.ones(len(nt), dtype=bool)
    if min_triangles is not None:
        keep &= nt >= int(min_triangles)
    if min_area is not None:
        keep &= area >= float(min_area)
    if keep_largest is not None:
        first = np.lexsort((np.arange(len(nt)), -nt))[:int(keep_largest)]  # most triangles first, ties to the lower id
        among = np.zeros(len(nt), dtype=bool)
        among[first] = True
        keep &= among
    return keep


def clean_numpy(vertices, triangles, min_triangles=None, min_area=None, keep_largest=None, remove_unreferenced=True, attributes=()):
    """Step 4 -> (vertices (M',3) float32, triangles (T',3) int32, the attributes' kept rows (list), vertex_remap (M) int32,
    kept_triangles (T') int32)."""
    vertices, tri = np.asarray(to_numpy(vertices)), np.asarray(to_numpy(triangles))
    attributes = [np.asarray(to_numpy(a)) for a in attributes]
    M, T = check_mesh(vertices, tri, tuple((f"attributes[{i}]", a) for i, a in enumerate(attributes)))
    keep_t = np.ones(T, dtype=bool)
    if _check_criteria(min_triangles, min_area, keep_largest):
        table = component_table_numpy(vertices, tri)
        keep_t = keep_components(table.num_triangles, table.area, min_triangles, min_area, keep_largest)[table.triangle_component]
    kept = np.nonzero(keep_t)[0].astype(np.int32)
    keep_v = np.ones(M, dtype=bool)
    if remove_unreferenced:
        keep_v[:] = False
        keep_v[tri[kept].astype(np.int64).ravel()] = True
    remap = np.where(keep_v, np.cumsum(keep_v) - 1, -1).astype(np.int32)
    return vertices[keep_v], remap[tri[kept].astype(np.int64)].reshape(-1, 3), [a[keep_v] for a in attributes], remap, kept


def vertex_normals_numpy(vertices, triangles):
    """Step 5 in float64 -> (M,3) float64 (the public form rounds to float32)."""
    vertices, tri = np.asarray(to_numpy(vertices)), np.asarray(to_numpy(triangles))
    M, T = check_mesh(vertices, tri)
    n = cross_numpy(vertices, tri)
    corner = tri.astype(np.int64).ravel()  # corner 3 t + k names vertex triangles[t][k]: ascending (t, k)
    # bincount adds in the order of the list: per vertex in ascending (triangle, corner)
    with np.errstate(all="ignore"):
        s = np.stack([np.bincount(corner, weights=np.repeat(n[:, c], 3), minlength=M) for c in range(3)], axis=1) if T else np.zeros((M, 3))
        length = _length(s)
        good = (length > 0) & np.isfinite(length)
        return np.where(good[:, None], s / np.where(good, length, 1.0)[:, None], 0.0)


# ---- the device path ---------------------------------------------------------------------------------------------------------------------
def _labels_device(tri, M):
    """The host-driven rounds -> (label, referenced, rounds).  The changed word is read after every round (one 4-byte copy): reading
    it every second round instead was not worth an extra round (profiles/mesh_clean.txt)."""
    import torch
    from . import ops
    dev = tri.device
    label = torch.empty(M, dtype=torch.int32, device=dev)
    referenced = torch.empty(M, dtype=torch.uint8, device=dev)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    cap = max_rounds(M)
    for rounds in range(1, cap + 1):
        ops.mesh_hook_round(tri, M, label, referenced, changed, first=rounds == 1)
        if tri.shape[0] == 0 or int(changed.item()) == 0:
            return label, referenced, rounds
    raise RuntimeError(f"the labelling did not converge within {cap} rounds")


def _components_device(vertices, tri):
    import torch
    from . import ops
    M = int(vertices.shape[0])
    label, referenced, rounds = _labels_device(tri, M)
    vcomp, num = ops.mesh_component_rank(label, referenced)
    C = int(num.item())
    tcomp, nv = ops.mesh_component_table(vcomp, tri, C)
    key, perm = torch.sort(tcomp, stable=True)
    nt, area = ops.mesh_component_sums(vertices, tri, key, perm, C)
    return MeshComponents(vcomp, tcomp, nt, nv, area, rounds)


# ---- public --------------------------------------------------------------------------------------------------------------------------
def mesh_components(mesh, triangles=None):
    """-> MeshComponents (steps 1 to 3).  mesh: a Mesh, a pair (vertices, triangles), or the vertices with triangles=.  Arrays on the
    host run the numpy forms; GPU tensors run the kernels and give GPU tensors."""
    vertices, triangles, _ = split_mesh(mesh, triangles)
    place = one_place(vertices, triangles, what="mesh arrays")
    check_mesh(vertices, triangles)
    if place == "host":
        return component_table_numpy(vertices, triangles)
    return _components_device(vertices.contiguous(), int32_triangles(triangles))


def clean_mesh(mesh, min_triangles=None, min_area=None, keep_largest=None, remove_unreferenced=True, attributes=None, details=False):
    """Step 4 -> a new Mesh (its colors and normals follow their vertices).  attributes: per-vertex (M,k) float32 arrays, a list or a
    dict of them.  With attributes or details=True the result is a CleanResult: the mesh, the attributes' kept rows in the same
    container, vertex_remap and kept_triangles.  Arrays on the host run clean_numpy; GPU tensors run the kernels: the table's counts
    and areas (C values each) are read for the verdicts, the two output sizes for the allocation."""
    if not is_mesh(mesh):
        mesh = Mesh(*split_mesh(mesh)[:2])
    has_criteria = _check_criteria(min_triangles, min_area, keep_largest)
    names = list(attributes) if isinstance(attributes, dict) else None
    given = [] if attributes is None else list(attributes.values() if names is not None else attributes)
    own = [(n, getattr(mesh, n, None)) for n in ("colors", "normals")]
    rows = [a for _, a in own if a is not None] + given
    labels = [f"mesh.{n}" for n, a in own if a is not None] + [f"attributes[{i if names is None else repr(names[i])}]" for i in range(len(given))]
    place = one_place(mesh.vertices, mesh.triangles, *rows, what="mesh arrays")
    M, T = check_mesh(mesh.vertices, mesh.triangles, tuple(zip(labels, rows)))
    if place == "host":
        v, t, out, remap, kept = clean_numpy(mesh.vertices, mesh.triangles, min_triangles, min_area, keep_largest, remove_unreferenced, rows)
    else:
        import torch
        from . import ops
        vertices, tri = mesh.vertices.contiguous(), int32_triangles(mesh.triangles)
        tcomp = keep = None
        if has_criteria:
            table = _components_device(vertices, tri)
            verdict = keep_components(table.num_triangles.cpu().numpy(), table.area.cpu().numpy(), min_triangles, min_area, keep_largest)
            tcomp, keep = table.triangle_component, torch.from_numpy(verdict.astype(np.uint8)).to(vertices.device)
        t, kept, remap, Mk = ops.mesh_filter(tri, M, tcomp, keep, remove_unreferenced)
        v = ops.mesh_gather_rows(vertices, remap, Mk)
        out = [ops.mesh_gather_rows(a.contiguous(), remap, Mk) for a in rows]
    out = list(out)
    new = Mesh(v, t)
    for n, a in own:
        if a is not None:
            setattr(new, n, out.pop(0))
    if attributes is None and not details:
        return new
    attrs = None if attributes is None else (dict(zip(names, out)) if names is not None else out)
    return CleanResult(new, attrs, remap, kept)


def vertex_normals(mesh, triangles=None):
    """Step 5 -> (M,3) float32: numpy on the host, the kernel (and a GPU tensor) for a mesh on a GPU."""
    vertices, triangles, _ = split_mesh(mesh, triangles)
    place = one_place(vertices, triangles, what="mesh arrays")
    check_mesh(vertices, triangles)
    if place == "host":
        return vertex_normals_numpy(vertices, triangles).astype(np.float32)
    import torch
    from . import ops
    tri = int32_triangles(triangles)
    key, perm = torch.sort(tri.reshape(-1), stable=True)
    return ops.mesh_vertex_normals(vertices.contiguous(), tri, key, perm)
