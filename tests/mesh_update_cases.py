"""The meshes and scenes of the agpt_scene_update_mesh tests (test_mesh_update_api.py on the CPU, test_gpu_mesh_update.py on the GPU):
blobs of the same segment counts -- the same indices and texture coordinates -- in several poses."""
import numpy as np

import ag_pathtracer_amd as ag

F = np.float32
SEG, RING = 24, 16   # 768 triangles


def collapse(verts, indices, tri):
    """a zero-area triangle: its second vertex moved onto its first"""
    v = verts.copy()
    ix = np.asarray(indices).reshape(-1, 3)
    v[ix[3 * tri + 1, 0]] = v[ix[3 * tri, 0]]
    return v


def blob(pose, with_normals=True):
    """pose 0: the build pose; 1: another seed, radius and centre; both with one zero-area triangle, a different one each"""
    seed, radius, center, flat = [(3, 1.0, (0.0, 0.2, 0.0), 100), (8, 1.15, (0.3, 0.35, -0.2), 300)][pose]
    v, n, t, idx = ag.scenes.blob_mesh(SEG, RING, center=center, radius=radius, seed=seed)
    return collapse(v, idx, flat), (n if with_normals else None), t, idx


def scene(pose_a, pose_b, scale=1.0, backdrop=None, mpn=(1, 4)):
    """C1-style: backdrop, a Disney blob with normals (prim 1, max_prims_in_node 1), a mirror blob without (prim 2, max_prims_in_node
    4; `mpn` changes the two), sphere light, sky.  scale multiplies the positions of both blobs."""
    d = ag.SceneDesc("mesh-update")
    floor = d.add_material(ag.MAT_DISNEY, [.6, .62, .45], 1.0, 0.0)
    gold = d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], 0.4, 1.0)
    mirror = d.add_material(ag.MAT_MIRROR, [.9, .9, .9])
    v, n, t, idx = backdrop if backdrop is not None else ag.create_backdrop([0, -1.5, 20], [40, 20, 40], 7.5, 8)
    d.add_mesh(v, n, t, idx, floor, 1)
    va, na, ta, ia = blob(pose_a)
    d.add_mesh(va * F(scale), na, ta, ia, gold, mpn[0])
    vb, nb, tb, ib = blob(pose_b, with_normals=False)
    d.add_mesh((vb + np.array([2.4, 0, 0.5], F)) * F(scale), nb, tb, ib, mirror, mpn[1])
    d.add_area_light([0, 25, -20], 1.0, np.array([200, 188, 183], F))
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 2.0, -7.5], [1.0, 0.2, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d


def blob_arrays(d, prim):
    op = [o for o in d.ops if o[0] in ("mesh", "sphere", "plane", "area_light")][prim]
    return op[1], op[2]
