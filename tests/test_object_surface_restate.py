"""The referee of ``field.object_surfaces`` (tests/_object_surface_restate.py) is a sound yardstick on the inputs the GPU tests use:
closed meshes are watertight and outward, open ones are not, and neighbouring objects each get their own vertex on a shared edge."""
import numpy as np

import _object_surface_restate as OS
import _surface_restate as S


def undirected_use(faces):
    use = {}
    for (a, b), n in S.edge_use(faces).items():
        e = (min(a, b), max(a, b))
        use[e] = use.get(e, 0) + n
    return use


def check_closed(objects, cell=(1.0, 1.0, 1.0)):
    m = OS.measures(objects, cell)
    n = 0
    for k, (v, f) in enumerate(objects):
        if len(f) == 0:
            continue
        n += 1
        assert set(undirected_use(f).values()) == {2}, k                # every edge used exactly twice
        assert all(c == 1 for c in S.edge_use(f).values()), k           # ... once in each direction: consistently wound
        assert m["volume"][k] > 0 and m["area"][k] > 0, k
    return n


def test_closed_meshes_are_watertight_even_on_the_box_faces():
    labels, value, C = OS.box_objects()
    r = OS.object_surfaces(labels, value, C, 0.45, closed=True)
    assert check_closed(r.objects) == 3
    assert r.vertex_offset[-1] == len(r.vertices) and r.face_offset[-1] == len(r.faces)
    assert r.vertices.min() < 0                                          # object 0 touches the box: its surface lies in the border layer
    # vertex_cell names a cell of the vertex's own object
    for k in range(C):
        cells = r.vertex_cell[r.vertex_offset[k]:r.vertex_offset[k + 1]]
        assert np.all(labels.reshape(-1)[cells] == k)


def test_open_meshes_have_boundary_edges_where_the_object_touches_the_box():
    labels, value, C = OS.box_objects()
    r = OS.object_surfaces(labels, value, C, 0.45, closed=False)
    assert 1 in set(undirected_use(r.objects[0][1]).values())            # object 0 touches three box faces: the case `closed` exists for
    assert set(undirected_use(r.objects[2][1]).values()) == {2}          # the interior speck is closed either way
    c = OS.object_surfaces(labels, value, C, 0.45, closed=True)
    assert np.array_equal(c.objects[2][0], r.objects[2][0]) and np.array_equal(c.objects[2][1], r.objects[2][1])


def test_two_face_adjacent_objects_put_two_vertices_on_the_shared_edge():
    labels, value, C = OS.box_objects()
    r = OS.object_surfaces(labels, value, C, 0.45, closed=True)
    # the grid edge (2, 1, 1) -> (3, 1, 1) runs from object 0 into object 1, both inside
    on_edge = [[v for v in r.objects[k][0] if 2 < v[0] < 3 and v[1] == 1 and v[2] == 1] for k in (0, 1)]
    assert len(on_edge[0]) == 1 and len(on_edge[1]) == 1
    f = np.float32
    assert on_edge[0][0][0] == f(f(2) + f(f(f(0.45) - f(0.8)) / f(f(0) - f(0.8))))      # object 0 sees fill at the far end
    assert on_edge[1][0][0] == f(f(2) + f(f(f(0.45) - f(0)) / f(f(0.7) - f(0))))        # ... and so does object 1 at the near end
    assert on_edge[0][0][0] != on_edge[1][0][0]


def test_voronoi_inputs_give_closed_meshes_and_skip_foreign_labels():
    for shape, C, present, seed in (((12, 10, 14), 14, 14, 1), ((10, 9, 11), 94, 9, 2)):
        labels, value = OS.voronoi(shape, C, present, seed)
        assert (labels == 255).any() and (labels == C + 3).any()
        r = OS.object_surfaces(labels, value, C, 0.45, closed=True)
        assert check_closed(r.objects, (0.5, 0.25, 0.125)) >= min(present, 5)
        absent = [k for k in range(C) if not (labels == k).any()]
        assert all(len(r.objects[k][0]) == 0 for k in absent)
        if C == 94:
            assert len(absent) >= 80
