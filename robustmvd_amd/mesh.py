"""The argument layer of the geometry front ends (depth_fusion, cloud_eval, cloud_register, tsdf, render, mesh_clean, mesh_eval,
mesh_simplify): where an array lives, the Mesh container, the three forms a mesh argument takes, and the one check of a mesh's
arrays.  Everything here works on numpy arrays and torch tensors alike and imports nothing of the package at module level."""
from dataclasses import dataclass

import numpy as np

INTEGER_DTYPES = ("int32", "int64", "int16", "uint8", "int8", "uint16", "uint32", "uint64")


def is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def place(a):
    """"host" for a numpy array or a CPU tensor, else the GPU's name ("cuda:0")."""
    return str(a.device) if is_tensor(a) and a.is_cuda else "host"


def to_numpy(a):
    return a.detach().cpu().numpy() if is_tensor(a) else np.asarray(a)


def one_place(*arrays, what="arrays"):
    """-> the place all the arrays share; ValueError when they are in different places."""
    places = {place(a) for a in arrays}
    if len(places) != 1:
        raise ValueError(f"the {what} are in different places ({sorted(places)}): move them to one first")
    return places.pop()


def dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def int32_triangles(triangles):
    """A GPU mesh's triangles as the kernels take them."""
    import torch
    return triangles.to(torch.int32).contiguous()


@dataclass
class Mesh:
    """vertices (M,3) float32, triangles (T,3) int32 into them, colors (M,3) float32 or None, normals (M,3) float32 or None (nobody
    fills them in unasked: mesh.normals = mesh.vertex_normals()); numpy arrays from a volume on the host, GPU tensors from one on a
    GPU.  write_ply(path, mesh.vertices, mesh.colors, faces=mesh.triangles, normals=mesh.normals) saves it."""
    vertices: object
    triangles: object
    colors: object = None
    normals: object = None

    def render(self, intrinsics, poses, size, **kw):
        """-> RenderResult: the mesh seen from V views of one size (render.render_mesh; colors=True renders the mesh's own)."""
        from .render import render_mesh
        return render_mesh(self, intrinsics, poses, size, **kw)

    def components(self):
        """-> MeshComponents: the connected components with their counts and areas (mesh_clean.mesh_components)."""
        from .mesh_clean import mesh_components
        return mesh_components(self)

    def clean(self, **kw):
        """-> Mesh without the components that fail min_triangles=, min_area= or keep_largest= (mesh_clean.clean_mesh); with
        attributes= or details=True a CleanResult, whose .mesh is that Mesh."""
        from .mesh_clean import clean_mesh
        return clean_mesh(self, **kw)

    def simplify(self, cell, **kw):
        """-> Mesh with one vertex per occupied cell of edge `cell`, placed by the cell's quadric (mesh_simplify.simplify_mesh:
        placement=, regularisation=, origin=, unique=, remove_unreferenced=); with attributes= or details=True a SimplifyResult,
        whose .mesh is that Mesh."""
        from .mesh_simplify import simplify_mesh
        return simplify_mesh(self, cell, **kw)

    def vertex_normals(self):
        """-> (M,3) float32: the area-weighted vertex normals (mesh_clean.vertex_normals)."""
        from .mesh_clean import vertex_normals
        return vertex_normals(self)

    def distance(self, points, max_dist):
        """-> (dist (n) float32, index (n) int32): the truncated distance of every point to the surface and its nearest triangle, -1
        where nothing is nearer than max_dist (mesh_eval.mesh_distance)."""
        from .mesh_eval import mesh_distance
        return mesh_distance(points, self, max_dist)

    def sample(self, spacing, colors=False):
        """-> (points (S,3) float32, triangle (S) int32, colors (S,3) or None): covering samples of the surface, every surface point
        within 2 spacing / 3 of one (mesh_eval.sample_mesh); colors=True interpolates the mesh's vertex colours."""
        from .mesh_eval import sample_mesh
        if colors and self.colors is None:
            raise ValueError("Mesh.sample(colors=True): the mesh has no colours")
        return sample_mesh(self, spacing, self.colors if colors else None)


def is_mesh(obj):
    return hasattr(obj, "vertices") and hasattr(obj, "triangles")


def split_mesh(mesh, triangles=None, colors=None, required=True):
    """The three forms of a mesh argument -> (vertices, triangles, colors): a Mesh (anything with .vertices and .triangles), a pair
    (vertices, triangles), or the vertices with triangles=.  colors: None or False, the (M,3) array, or True for a Mesh's own.
    required=False gives None for anything else (a cloud) instead of a ValueError."""
    if is_mesh(mesh):
        if triangles is not None:
            raise ValueError("a Mesh brings its own triangles")
        return mesh.vertices, mesh.triangles, mesh.colors if colors is True else (None if colors is None or colors is False else colors)
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2 and triangles is None:
        mesh, triangles = mesh
    if triangles is None:
        if not required:
            return None
        raise ValueError(f"expected a Mesh, (vertices, triangles) or vertices with triangles=, got {type(mesh).__name__}")
    if colors is True:
        raise ValueError("colors=True needs a Mesh with colours; pass the (M,3) array instead")
    return mesh, triangles, None if colors is False else colors


def check_triangles(triangles, M, dtypes=True, index_range=True):
    """check_mesh's triangle half, for a caller that has M alone -> T."""
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError(f"triangles must be (T,3), got {tuple(triangles.shape)}")
    if dtypes and dtype_name(triangles) not in INTEGER_DTYPES:
        raise ValueError(f"triangles: dtype {dtype_name(triangles)}, expected an integer dtype (int32)")
    M, T = int(M), int(triangles.shape[0])
    if T >= 2 ** 31 or M >= 2 ** 31 or M < 0:
        raise ValueError(f"{M} vertices and {T} triangles: both must be below 2^31")
    if index_range and T:
        if is_tensor(triangles):
            import torch
            lo, hi = (int(x) for x in torch.aminmax(triangles))  # one reduction, one read of two numbers
        else:
            lo, hi = int(triangles.min()), int(triangles.max())
        if lo < 0 or hi >= M:
            raise ValueError(f"triangles: vertex indices must be in 0 .. {M - 1}, found {lo if lo < 0 else hi}")
    return T


def check_mesh(vertices, triangles, extra=(), dtypes=True, index_range=True):
    """The one check of a mesh's arrays -> (M, T): vertices (M,3), triangles (T,3), M and T below 2^31, every index in 0 .. M-1, and
    each (name, array) of extra a per-vertex (M,k) array.  dtypes: float32 vertices and extras and triangles of an integer dtype;
    False where the caller converts.  index_range: False where an index out of range only makes the triangle invalid (mesh_eval) or
    the caller has checked already (the per-launch wrappers of ops: the check reads the device)."""
    for name, a in (("vertices", vertices), ("triangles", triangles)) + tuple(extra):
        if not (is_tensor(a) or isinstance(a, np.ndarray)):
            raise ValueError(f"{name}: expected a numpy array or a torch tensor, got {type(a).__name__}")
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be (M,3), got {tuple(vertices.shape)}")
    if dtypes and dtype_name(vertices) != "float32":
        raise ValueError(f"vertices: dtype {dtype_name(vertices)}, expected float32")
    M = int(vertices.shape[0])
    T = check_triangles(triangles, M, dtypes, index_range)
    for name, a in extra:
        if a.ndim != 2 or a.shape[0] != M or a.shape[1] < 1 or (dtypes and dtype_name(a) != "float32"):
            raise ValueError(f"{name}: expected ({M},k) float32, got {tuple(a.shape)} {dtype_name(a)}")
    return M, T
