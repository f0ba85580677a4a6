"""A rig of unequal cameras: 16 cameras on a Fibonacci cap over the top point of the dome object (polar angle <= 25 degrees,
distance 4, tests/test_camera_sweep.py's cap_scene recipe), cycled through eight shape classes -- landscape and portrait,
odd sizes, fx != fy, calibrated (non-integer, off-centre) principal points, and images from 96 x 72 to 480 x 360.  The focal
length scales with the image size, so the object fills each view alike.

A plain module like tests/refcost.py: the rig, its seed maker (synth._make_seeds wants a 40-pixel margin in every camera and
cannot seed a 96 x 72 image), and the hand-built patch states of tests/test_mixed_rig.py.
"""
import math

import numpy as np

TOP = np.array([0.0, 0.0, 0.95])        # the top point of the dome object (its upper ellipsoid: z = 0.55 + 0.4)
N_CAMS = 16
# (width, height, (fx, fy), principal point or None for the (w >> 1, h >> 1) default)
SHAPES = ((320, 240, (400.0, 400.0), None),
          (240, 320, (400.0, 400.0), None),
          (333, 251, (416.0, 416.0), (160.37, 131.81)),
          (320, 240, (400.0, 433.0), (171.5, 109.25)),
          (160, 120, (200.0, 200.0), None),
          (480, 360, (600.0, 600.0), None),
          (96, 72, (120.0, 120.0), None),
          (257, 193, (330.0, 318.0), (120.2, 99.9)))
LANDSCAPE, PORTRAIT, ODD_PP, FX_FY, SMALL, LARGE, TINY, ODD_FXY = range(8)


def shape_class(cam_index):
    return cam_index % len(SHAPES)


def rig_scene(lod_ratio=0.8, cfg_max_lod=15, dist=4.0, max_polar_deg=25.0, tex_seed=4567, n_seeds=12, radius=7):
    """The rig with its pyramids built for (lod_ratio, cfg_max_lod) and n_seeds seeds that keep every visible camera."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.camera import Camera, quaternion_to_rotation, rotation_to_quaternion
    up = np.array([0.0, 0.0, 1.0])
    parts = [synth.Ellipsoid(-0.35, 0.75, 0.3), synth.Ellipsoid(0.0, 0.5, 0.7), synth.Ellipsoid(0.55, 0.4, 0.4)]
    rng = np.random.default_rng(tex_seed)
    px = dist / 400.0
    k, phi, amp = synth.make_texture(rng, 32, 7 * px, 40 * px, 34.0)
    obj = synth.SolidOfRevolution(np.zeros(3), up, parts, k, phi, amp)
    cams = []
    ga = math.pi * (3 - math.sqrt(5))
    c0 = math.cos(math.radians(max_polar_deg))
    for i in range(N_CAMS):
        w, h, f, pp = SHAPES[shape_class(i)]
        zc = 1.0 - (1.0 - c0) * (i + 0.5) / N_CAMS
        rr = math.sqrt(1 - zc * zc)
        C = TOP + dist * np.array([rr * math.cos(ga * i), rr * math.sin(ga * i), zc])
        q = rotation_to_quaternion(synth._look_at(C, TOP.copy(), np.array([0.0, 1.0, 0.0])))
        f2 = np.array(f)
        pp2 = np.array(pp) if pp else np.array([float(w >> 1), float(h >> 1)])
        img = synth.render(obj, quaternion_to_rotation(q), C, f2, pp2, w, h)
        cams.append(Camera(focal=f2, principle_point=np.array(pp) if pp else np.array([-1.0, -1.0]), quaternion=q, center=C,
                           image=img, name="mix%02d" % i).finalize(lod_ratio, cfg_max_lod, True))
    return synth.Scene("mixed", cams, obj, make_seeds(obj, cams, n_seeds, radius))


def with_pyramids(scene, lod_ratio, cfg_max_lod):
    """The same cameras, images and seeds with the pyramids of another (lodRatio, maxLOD)."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.camera import Camera
    cams = [Camera(focal=c.focal.copy(), principle_point=c.principle_point.copy(), quaternion=c.quaternion.copy(),
                   center=c.center.copy(), image=c.image, name=c.name).finalize(lod_ratio, cfg_max_lod, True) for c in scene.cameras]
    return synth.Scene(scene.name, cams, scene.obj, scene.seeds)


def project0(cam, X):
    Xc = cam.rotation @ np.asarray(X, float) + cam.translation
    return (float(cam.focal[0] * Xc[0] / Xc[2] + cam.principle_point[0]), float(cam.focal[1] * Xc[1] / Xc[2] + cam.principle_point[1]))


def visible_cams(obj, X, normal, cams, margin, min_cos=0.35):
    """synth._visible_cams with the margin in pixels of each camera's own image."""
    vis = []
    for i, c in enumerate(cams):
        v = X - c.center
        dist = np.linalg.norm(v)
        d = v / dist
        if -(d @ normal) < min_cos:
            continue
        t = obj.intersect(c.center, d[None, :])[0]
        if not np.isfinite(t) or abs(t - dist) > 1e-6 * max(1.0, dist):
            continue
        u, v2 = project0(c, X)
        if margin <= u < c.width - margin and margin <= v2 < c.height - margin:
            vis.append(i)
    return vis


def surface_point(x, y):
    """The point of the upper ellipsoid (a sphere of radius 0.4 around (0, 0, 0.55)) above (x, y)."""
    return np.array([x, y, 0.55 + math.sqrt(0.16 - x * x - y * y)])


def make_seeds(obj, cams, n_seeds, radius):
    """Surface points on a golden-angle spiral around the top point, each with the cameras into whose own image it projects
    at least radius + 6 pixels inside."""
    from pais_mvs_amd import synth
    seeds = []
    ga = math.pi * (3 - math.sqrt(5))
    for i in range(n_seeds):
        rho = 0.12 * math.sqrt((i + 0.5) / n_seeds)
        X = surface_point(rho * math.cos(ga * i), rho * math.sin(ga * i))
        vis = visible_cams(obj, X, synth._surface_normal(obj, X), cams, radius + 6)
        seeds.append((X, vis))
    return seeds


def highest_fitting_lod(cam, X, lod_ratio, radius):
    """The highest level of cam at which the window of radius `radius` around the projection of X passes patch.cpp:957-962."""
    u, v = project0(cam, X)
    best = -1
    for lod in range(cam.max_lod + 1):
        rows, cols = cam.pyramid[lod].shape
        s = lod_ratio ** lod
        if u * s - radius >= 2 and u * s + radius < cols - 3 and v * s - radius >= 2 and v * s + radius < rows - 3:
            best = lod
    return best
