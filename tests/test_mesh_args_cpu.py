"""The argument layer the mesh front ends share, on the host: every input form a front end documents (a Mesh, a (vertices,
triangles) pair, vertices with triangles=) gives identical results, and a table of malformed meshes is accepted or refused by
each front end exactly as recorded here.  The table holds literals: it was recorded before the front ends shared their argument
code and pins what each of them did then, differences included."""
import dataclasses

import numpy as np
import pytest

import robustmvd_amd as R


def tetrahedra():
    """Two disconnected tetrahedra (8 vertices, 8 triangles, outward winding) with colours."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)
    vertices = np.concatenate([v, 0.5 * v + np.float32(3)]) * np.float32(0.25)
    colors = np.linspace(0.0, 1.0, 24, dtype=np.float32).reshape(8, 3)
    return vertices, np.concatenate([t, t + 4]), colors


VIEW = ([np.array([[8.0, 0, 3.5], [0, 8.0, 3.5], [0, 0, 1]])], [np.array([[1.0, 0, 0, -0.3], [0, 1, 0, -0.3], [0, 0, 1, 1.5], [0, 0, 0, 1]])],
        (8, 8))
QUERY = np.array([[0.1, 0.1, 0.3], [0.9, 0.8, 0.8], [5.0, 5.0, 5.0]], dtype=np.float32)


def same(a, b):
    if dataclasses.is_dataclass(a):
        return type(a) is type(b) and all(same(getattr(a, f.name), getattr(b, f.name)) for f in dataclasses.fields(a))
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b


# name -> (call(mesh, **triangles), the forms it documents)
FRONT_ENDS = {
    "mesh_components": (lambda m, **kw: R.mesh_components(m, **kw), ("mesh", "pair", "list", "keyword")),
    "vertex_normals": (lambda m, **kw: R.vertex_normals(m, **kw), ("mesh", "pair", "list", "keyword")),
    "clean_mesh": (lambda m: R.clean_mesh(m, keep_largest=1, details=True), ("mesh", "pair", "list")),
    "render_mesh": (lambda m, **kw: R.render_mesh(m, *VIEW, normals=True, bary=True, **kw), ("mesh", "pair", "list", "keyword")),
    "mesh_distance": (lambda m: R.mesh_distance(QUERY, m, 0.5), ("mesh", "pair", "list")),
    "sample_mesh": (lambda m: R.sample_mesh(m, 0.1), ("mesh", "pair", "list")),
    "simplify_mesh": (lambda m: R.simplify_mesh(m, 0.2, details=True), ("mesh", "pair", "list")),
    "evaluate_pred": (lambda m: R.MeshEvaluation((0.05, 0.1))(m, QUERY), ("mesh", "pair", "list")),
    "evaluate_gt": (lambda m: R.MeshEvaluation((0.05, 0.1))(QUERY, m), ("mesh", "pair", "list")),
}


def in_form(form, v, t):
    """-> (args, kwargs) of one input form"""
    if form == "keyword":
        return (v,), {"triangles": t}
    return ({"mesh": R.Mesh(v, t), "pair": (v, t), "list": [v, t]}[form],), {}


@pytest.mark.parametrize("name", sorted(FRONT_ENDS))
def test_every_input_form_gives_the_same_result(name):
    v, t, _ = tetrahedra()
    call, forms = FRONT_ENDS[name]
    results = []
    for form in forms:
        args, kwargs = in_form(form, v, t)
        results.append(call(*args, **kwargs))
    assert len(results) >= 3
    for form, r in zip(forms[1:], results[1:]):
        assert same(results[0], r), form


def test_a_mesh_brings_its_colours_and_normals():
    v, t, c = tetrahedra()
    mesh = R.Mesh(v, t, c)
    own = R.render_mesh(mesh, *VIEW, colors=True)
    assert own.colors is not None and own.mask[0].any()
    assert same(own, R.render_mesh((v, t), *VIEW, colors=c)) and same(own, R.render_mesh(v, *VIEW, triangles=t, colors=c))
    assert same(own, R.render_mesh(mesh, *VIEW, colors=c))
    for off in (None, False):
        assert R.render_mesh(mesh, *VIEW, colors=off).colors is None and R.render_mesh((v, t), *VIEW, colors=off).colors is None
    # a pair carries no colours: clean_mesh and simplify_mesh take them as attributes, with the same rows
    cleaned = R.clean_mesh(mesh, keep_largest=1)
    by_attribute = R.clean_mesh((v, t), keep_largest=1, attributes=[c])
    assert same(cleaned.colors, by_attribute.attributes[0]) and same(cleaned.vertices, by_attribute.mesh.vertices)
    simple = R.simplify_mesh(mesh, 0.2)
    by_attribute = R.simplify_mesh((v, t), 0.2, attributes={"c": c})
    assert same(simple.colors, by_attribute.attributes["c"]) and same(simple.triangles, by_attribute.mesh.triangles)
    with_normals = R.Mesh(v, t, normals=R.vertex_normals(v, t))
    assert same(R.render_mesh(with_normals, *VIEW, normals="vertex"), R.render_mesh((v, t), *VIEW, normals="vertex"))


def test_the_mesh_methods_are_the_front_ends():
    v, t, c = tetrahedra()
    mesh = R.Mesh(v, t, c)
    assert R.Mesh is R.tsdf.Mesh
    assert same(mesh.components(), R.mesh_components(mesh))
    assert same(mesh.vertex_normals(), R.vertex_normals(v, t))
    assert same(mesh.clean(keep_largest=1), R.clean_mesh(mesh, keep_largest=1))
    assert same(mesh.simplify(0.2), R.simplify_mesh(mesh, 0.2))
    assert same(mesh.render(*VIEW, colors=True), R.render_mesh(mesh, *VIEW, colors=True))
    assert same(mesh.distance(QUERY, 0.5), R.mesh_distance(QUERY, (v, t), 0.5))
    assert same(mesh.sample(0.1), R.sample_mesh((v, t), 0.1))
    assert same(mesh.sample(0.1, colors=True), R.sample_mesh((v, t), 0.1, c))
    both = R.MeshEvaluation((0.05, 0.1))(mesh, (v + np.float32(0.01), t))
    assert same(both, R.MeshEvaluation((0.05, 0.1))([v, t], R.Mesh(v + np.float32(0.01), t)))
    assert both.fscore[1] > 0.99


def bad_mesh(kind):
    v, t, _ = tetrahedra()
    if kind == "vertices (M,2)":
        return v[:, :2], t
    if kind == "triangles (T,4)":
        return v, np.concatenate([t, t[:, :1]], axis=1)
    if kind == "float triangles":
        return v, t.astype(np.float32)
    if kind == "index M":
        t = t.copy()
        t[5, 1] = len(v)
        return v, t
    if kind == "negative index":
        t = t.copy()
        t[5, 1] = -1
        return v, t
    if kind == "float64 vertices":
        return v.astype(np.float64), t
    if kind == "empty triangles":
        return v, np.zeros(0, dtype=np.int32)
    if kind == "empty (0,3) triangles":
        return v, np.zeros((0, 3), dtype=np.int32)
    raise KeyError(kind)


KINDS = ("vertices (M,2)", "triangles (T,4)", "float triangles", "index M", "negative index", "float64 vertices", "empty triangles",
         "empty (0,3) triangles")
# what each front end did with each kind before the argument code was shared: "R" refuses with ValueError, "A" accepts
#                                        (M,2)  (T,4)  float t  idx M  idx<0  f64 v  empty  (0,3)
OUTCOMES = {"mesh_components": "R      R      R        R      R      R      R      A",
            "vertex_normals":  "R      R      R        R      R      R      R      A",
            "clean_mesh":      "R      R      R        R      R      R      R      A",
            "simplify_mesh":   "R      R      R        R      R      R      R      A",
            "render_mesh":     "R      R      A        R      R      A      R      A",
            "mesh_distance":   "R      R      R        A      A      A      A      A",
            "sample_mesh":     "R      R      R        A      A      A      A      A",
            "evaluate_pred":   "R      R      R        A      A      A      A      A",
            "evaluate_gt":     "R      R      R        A      A      A      A      A"}


@pytest.mark.parametrize("name", sorted(FRONT_ENDS))
def test_malformed_meshes_meet_the_recorded_outcome(name):
    assert sorted(OUTCOMES) == sorted(FRONT_ENDS)
    call, _ = FRONT_ENDS[name]
    for kind, expected in zip(KINDS, OUTCOMES[name].split(), strict=True):
        if expected == "R":
            with pytest.raises(ValueError):
                call(bad_mesh(kind))
        else:
            call(bad_mesh(kind))


def test_colors_true_needs_a_mesh():
    v, t, c = tetrahedra()
    with pytest.raises(ValueError, match="colours"):
        R.render_mesh((v, t), *VIEW, colors=True)
    with pytest.raises(ValueError, match="colours"):
        R.render_mesh(v, *VIEW, triangles=t, colors=True)
    with pytest.raises(ValueError, match="colours"):
        R.Mesh(v, t).sample(0.1, colors=True)
    assert R.render_mesh(R.Mesh(v, t), *VIEW, colors=True).colors is None  # a Mesh without colours renders without
    with pytest.raises(ValueError, match="own triangles"):
        R.render_mesh(R.Mesh(v, t, c), *VIEW, triangles=t)
    for refuses in (lambda: R.vertex_normals(v), lambda: R.clean_mesh(v), lambda: R.simplify_mesh(v, 0.2), lambda: R.sample_mesh(v, 0.1),
                    lambda: R.mesh_distance(QUERY, v, 0.5)):
        with pytest.raises(ValueError, match="expected a Mesh"):
            refuses()
