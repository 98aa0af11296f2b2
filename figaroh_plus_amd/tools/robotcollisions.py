"""Self-collision distances of primitive shapes: ``CollisionWrapper`` of src/figaroh/tools/robotcollisions.py:20-134 with the
geometry model it reads (pin.GeometryModel / pin.GeometryObject / pin.CollisionPair and the hpp-fcl shapes of
examples/tiago/utils/simplified_colission_model.py:27-180), without Pinocchio or hpp-fcl.

Distance convention.  Every shape is a convex *core* and a radius r: a ``Box`` or a ``Cylinder`` is its own core with r = 0,
the core of a ``Sphere`` is its centre, the core of a ``Capsule`` its axis segment.  The distance of a pair is

    d = dist(core_A, core_B) - r_A - r_B.

For separated shapes this is the Euclidean distance (hpp-fcl's ``min_distance``); for rounded shapes in shallow overlap it is
minus the penetration depth; when the cores themselves intersect it is exactly ``-(r_A + r_B)`` (<= 0) with status
``STATUS_CORES_INTERSECT`` -- hpp-fcl would run EPA there and return a depth, which is not mirrored: the optimiser's bound is
d >= 0.01, so any non-positive value is a violation either way.

Algorithm (``collision_distances_mirror`` here, ``figh_collision_distances`` in csrc/figh_collision.hip, statement for
statement).  The world placement of a geometry is oM_parent . placement.  GJK runs in the world frame on the Minkowski
difference core_A - core_B with closed-form support functions:
  box       (+-hx, +-hy, +-hz) by the signs of the direction, a zero (or -0.0) component takes +h;
  cylinder  (r dx / d_xy, r dy / d_xy, +-hl) with d_xy = sqrt(dx^2 + dy^2); d_xy = 0 returns the cap centre (0, 0, +-hl);
            dz >= 0 takes +hl;
  sphere    the centre;   capsule  (0, 0, +-hl), dz >= 0 takes +hl.
The first direction is centre_A - centre_B, or (1, 0, 0) when that is zero.  Per step: w = s_A(-v) - s_B(v); with a simplex
in hand the step stops with ``STATUS_OK`` when |v| - v.w / |v| <= tol (v.w / |v| is a lower bound of the distance, |v| an upper
one); otherwise w joins the simplex (at most four points, each with its witness on A), the closest point of the simplex to
the origin is found by a case analysis over its sub-simplices (segment: clamped projection; triangle: the vertex, edge and
face regions in a fixed order; tetrahedron: the closest of the three faces that hold the new point, in a fixed order -- the
step that added the point has ruled the fourth out -- and "encloses the origin" when the origin lies strictly on the inner
side of all four faces, a face whose opposite vertex is within 2^-40 of its plane, relative, never counting as inner, and
the step's lower bound v.w is not positive: a positive one is a separating plane, which no flat tetrahedron can talk away),
points of zero weight leave the simplex, and v becomes that closest point.  The query
ends with ``STATUS_CORES_INTERSECT`` when the simplex encloses the origin or |v| <= 2^-40 max |simplex point|, and with
``STATUS_ITERATION_CAP`` after ``max_iter`` support evaluations; then |v| is still an upper bound of the core distance.
The witnesses are p_A = sum lambda_i a_i and p_B = p_A - v (world frame, on the cores) and d = |p_A - p_B| - (r_A + r_B).

Display methods and SRDF pair removal are not mirrored.
"""
import numpy as np

from ..model import SE3

KIND_BOX, KIND_CYLINDER, KIND_SPHERE, KIND_CAPSULE = 0, 1, 2, 3
KIND_NAMES = ("box", "cylinder", "sphere", "capsule")
STATUS_OK, STATUS_CORES_INTERSECT, STATUS_ITERATION_CAP = 0, 1, 2
DEFAULT_TOL = 1e-9        # metres, absolute
DEFAULT_MAX_ITER = 128
MAX_GEOMETRIES, MAX_PAIRS = 16, 64   # what the argument block of figh_collision_distances holds (include/figh.h)
_ZERO_REL_SQ = 2.0 ** -80            # (2^-40)^2: |v|^2 against max |s_i|^2, a face's opposite vertex against its plane


# --------------------------------------------------------------------------------------------------------------- shapes
class Box:
    """hppfcl.Box(x, y, z): full side lengths, centred."""
    kind = KIND_BOX

    def __init__(self, x, y, z):
        self.halfSide = np.array([x, y, z], dtype=np.float64) * 0.5
        self.dimensions = (float(x), float(y), float(z))
        self.core_radius = 0.0


class Cylinder:
    """hppfcl.Cylinder(radius, lz): axis z, centred, full length."""
    kind = KIND_CYLINDER

    def __init__(self, radius, length):
        self.radius, self.halfLength = float(radius), float(length) * 0.5
        self.dimensions = (float(radius), float(length))
        self.core_radius = 0.0


class Sphere:
    """hppfcl.Sphere(radius)."""
    kind = KIND_SPHERE

    def __init__(self, radius):
        self.radius = float(radius)
        self.dimensions = (float(radius),)
        self.core_radius = float(radius)


class Capsule:
    """hppfcl.Capsule(radius, lz): the points within ``radius`` of the centred z segment of full length ``length`` (the shape
    the reference wanted, simplified_colission_model.py:27-34, and replaced by a cylinder for an hpp-fcl bug)."""
    kind = KIND_CAPSULE

    def __init__(self, radius, length):
        self.radius, self.halfLength = float(radius), float(length) * 0.5
        self.dimensions = (float(radius), float(length))
        self.core_radius = float(radius)


_SHAPES = {"box": Box, "cylinder": Cylinder, "sphere": Sphere, "capsule": Capsule}


def _check_shape(shape):
    dims = np.asarray(shape.dimensions, dtype=np.float64)
    if not isinstance(shape, (Box, Cylinder, Sphere, Capsule)):
        raise TypeError("shape must be a Box, Cylinder, Sphere or Capsule (meshes are out of scope)")
    if not (np.all(np.isfinite(dims)) and np.all(dims >= 0.0)):
        raise ValueError("shape dimensions must be finite and non-negative, got %r" % (shape.dimensions,))


class GeometryObject:
    """pin.GeometryObject(name, parent_joint, shape, placement): ``placement`` (a ``model.SE3``) maps shape coordinates to
    the coordinates of joint ``parent_joint`` (0: the universe)."""

    def __init__(self, name, parent_joint, shape, placement=None):
        _check_shape(shape)
        self.name, self.parentJoint, self.geometry = str(name), int(parent_joint), shape
        self.placement = SE3() if placement is None else placement.copy()
        self.meshColor = np.array([0.7, 0.7, 0.98, 1.0])


class CollisionPair:
    """pin.CollisionPair(first, second): two geometry ids."""

    def __init__(self, first, second):
        self.first, self.second = int(first), int(second)
        if self.first == self.second:
            raise ValueError("a collision pair needs two different objects")

    def __eq__(self, other):
        return isinstance(other, CollisionPair) and {self.first, self.second} == {other.first, other.second}

    def __repr__(self):
        return "CollisionPair(%d, %d)" % (self.first, self.second)


class GeometryModel:
    """pin.GeometryModel restricted to primitives: ``geometryObjects`` and ``collisionPairs`` in insertion order."""

    def __init__(self):
        self.geometryObjects = []
        self.collisionPairs = []

    @property
    def ngeoms(self):
        return len(self.geometryObjects)

    def addGeometryObject(self, obj):
        if any(o.name == obj.name for o in self.geometryObjects):
            raise ValueError("a geometry object named %r is already in the model" % obj.name)
        self.geometryObjects.append(obj)
        return len(self.geometryObjects) - 1

    def getGeometryId(self, name):
        """The id of the object called ``name``; ``ngeoms`` when there is none (as Pinocchio)."""
        for i, o in enumerate(self.geometryObjects):
            if o.name == name:
                return i
        return len(self.geometryObjects)

    def existGeometryName(self, name):
        return self.getGeometryId(name) < len(self.geometryObjects)

    def addCollisionPair(self, pair):
        if not (0 <= pair.first < self.ngeoms and 0 <= pair.second < self.ngeoms):
            raise ValueError("%r names an object that is not in the model (%d objects)" % (pair, self.ngeoms))
        if pair not in self.collisionPairs:
            self.collisionPairs.append(pair)

    def addAllCollisionPairs(self):
        """Every pair of objects with different parent joints, first < second (pin.GeometryModel.addAllCollisionPairs)."""
        self.collisionPairs = []
        for i in range(self.ngeoms):
            for j in range(i + 1, self.ngeoms):
                if self.geometryObjects[i].parentJoint != self.geometryObjects[j].parentJoint:
                    self.collisionPairs.append(CollisionPair(i, j))

    def createData(self):
        return None  # (results live on the wrapper)

    def to_dict(self, model):
        """Settings only, parent joints by NAME: ``{"objects": [...], "pairs": [[first name, second name], ...]}``."""
        objs = []
        for o in self.geometryObjects:
            d = {"name": o.name, "parent_joint": model.names[o.parentJoint], "kind": KIND_NAMES[o.geometry.kind],
                 "dimensions": [float(x) for x in o.geometry.dimensions],
                 "translation": [float(x) for x in o.placement.translation]}
            if not np.array_equal(o.placement.rotation, np.eye(3)):
                d["rotation"] = [[float(x) for x in row] for row in o.placement.rotation]
            objs.append(d)
        names = [o.name for o in self.geometryObjects]
        return {"objects": objs, "pairs": [[names[p.first], names[p.second]] for p in self.collisionPairs]}

    @classmethod
    def from_dict(cls, d, model):
        gm = cls()
        for o in d["objects"]:
            if not model.existJointName(o["parent_joint"]):
                raise ValueError("geometry %r sits on joint %r, which the model does not have" % (o["name"], o["parent_joint"]))
            if o["kind"] not in _SHAPES:
                raise ValueError("geometry %r: unknown kind %r" % (o["name"], o["kind"]))
            gm.addGeometryObject(GeometryObject(o["name"], model.getJointId(o["parent_joint"]),
                                                _SHAPES[o["kind"]](*o["dimensions"]),
                                                SE3(o.get("rotation"), o.get("translation"))))
        for first, second in d["pairs"]:
            ids = gm.getGeometryId(first), gm.getGeometryId(second)
            if max(ids) >= gm.ngeoms:
                raise ValueError("pair (%r, %r) names an object that is not in the model" % (first, second))
            gm.addCollisionPair(CollisionPair(*ids))
        return gm


def geometry_table(geom_model):
    """(kind, parent, placement, dims, pairs, radius): the launch-uniform host arrays of ``figh_collision_distances`` --
    int32 kinds and parent joints, (n, 12) placements (rotation row-major, translation), (n, 3) dimensions as the shapes'
    constructors take them (full lengths), (n_pairs, 2) int32 object ids, and the core radii the entry derives from them."""
    objs = geom_model.geometryObjects
    n = len(objs)
    kind = np.array([o.geometry.kind for o in objs], dtype=np.int32).reshape(n)
    parent = np.array([o.parentJoint for o in objs], dtype=np.int32).reshape(n)
    placement = np.zeros((n, 12))
    dims = np.zeros((n, 3))
    for i, o in enumerate(objs):
        placement[i, :9] = np.asarray(o.placement.rotation, dtype=np.float64).reshape(9)
        placement[i, 9:] = o.placement.translation
        dims[i, :len(o.geometry.dimensions)] = o.geometry.dimensions
    pairs = np.array([[p.first, p.second] for p in geom_model.collisionPairs], dtype=np.int32).reshape(-1, 2)
    radius = np.array([o.geometry.core_radius for o in objs], dtype=np.float64).reshape(n)
    return kind, parent, placement, dims, pairs, radius


# ---------------------------------------------------------------------------------------------------------- host mirror
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)


def core_half_extents(kind, dims):
    """The three numbers the support function of a core reads, from a shape's constructor arguments: the box's half sides;
    (radius, half length, 0) of a cylinder; zeros for a sphere; (0, half length, 0) for a capsule."""
    if kind == KIND_BOX:
        return np.array([dims[0] * 0.5, dims[1] * 0.5, dims[2] * 0.5])
    if kind == KIND_CYLINDER:
        return np.array([dims[0], dims[1] * 0.5, 0.0])
    if kind == KIND_CAPSULE:
        return np.array([0.0, dims[1] * 0.5, 0.0])
    return np.zeros(3)


def _support_local(kind, h, d):
    """Support point of the core in the local direction d (M, 3)."""
    if kind == KIND_BOX:
        return np.where(d >= 0.0, h, -h)
    out = np.zeros_like(d)
    if kind == KIND_SPHERE:
        return out
    out[:, 2] = np.where(d[:, 2] >= 0.0, h[1], -h[1])
    if kind == KIND_CYLINDER:
        dxy = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        s = np.where(dxy > 0.0, h[0] / np.where(dxy > 0.0, dxy, 1.0), 0.0)
        out[:, 0], out[:, 1] = s * d[:, 0], s * d[:, 1]
    return out


def _support_world(kind, h, R, p, d):
    """R s(R^T d) + p."""
    dl = np.stack([R[:, 0, c] * d[:, 0] + R[:, 1, c] * d[:, 1] + R[:, 2, c] * d[:, 2] for c in range(3)], axis=-1)
    s = _support_local(kind, h, dl)
    return np.stack([R[:, r, 0] * s[:, 0] + R[:, r, 1] * s[:, 1] + R[:, r, 2] * s[:, 2] for r in range(3)], axis=-1) + p


def _closest_segment(a, b):
    """Weights (M, 2) of the point of the segment ab closest to the origin."""
    ab = b - a
    t, den = -_dot(a, ab), _dot(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(t <= 0.0, 0.0, np.where(t >= den, 1.0, t / den))
    return np.stack((1.0 - u, u), axis=-1)


def _closest_triangle(a, b, c):
    """Weights (M, 3) of the point of the triangle abc closest to the origin: the vertex regions of a, b, the edge ab, the
    vertex region of c, the edges ac, bc, the face, in this order."""
    ab, ac = b - a, c - a
    d1, d2 = -_dot(ab, a), -_dot(ac, a)
    d3, d4 = -_dot(ab, b), -_dot(ac, b)
    d5, d6 = -_dot(ab, c), -_dot(ac, c)
    # the face weights as triple products n . (x cross edge): equal to d1 d4 - d3 d2 and its two companions, which cancel badly
    # on the needle triangles of a converging query
    nrm = _cross(ab, ac)
    vc = _dot(nrm, _cross(a, ab))
    vb = _dot(nrm, _cross(ac, a))
    va = _dot(nrm, _cross(b, c - b))
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    fv, fw = vb * den, vc * den
    conds = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0),
             (d6 >= 0.0) & (d5 <= d6), (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0),
             (va <= 0.0) & (d4 - d3 >= 0.0) & (d5 - d6 >= 0.0)]
    l0 = np.select(conds, [one, zero, 1.0 - t_ab, zero, 1.0 - t_ac, zero], (1.0 - fv) - fw)
    l1 = np.select(conds, [zero, one, t_ab, zero, zero, 1.0 - t_bc], fv)
    l2 = np.select(conds, [zero, zero, zero, one, t_ac, t_bc], fw)
    return np.stack((l0, l1, l2), axis=-1)


_FACES = ((0, 1, 2, 3), (0, 1, 3, 2), (0, 2, 3, 1), (1, 2, 3, 0))  # three face vertices, the opposite vertex


def _closest_tetrahedron(S):
    """(weights (M, 4), encloses (M,)) for the tetrahedra S (M, 4, 3)."""
    M = S.shape[0]
    best = np.full(M, np.inf)
    lam = np.zeros((M, 4))
    inside = np.ones(M, dtype=bool)
    for i, j, k, o in _FACES:
        a, b, c, e = S[:, i], S[:, j], S[:, k], S[:, o]
        nrm = _cross(b - a, c - a)
        ea = e - a
        side_o, side_e = -_dot(a, nrm), _dot(ea, nrm)
        inside &= (side_o * side_e > 0.0) & (side_e * side_e > _ZERO_REL_SQ * (_dot(nrm, nrm) * _dot(ea, ea)))
        if o == 3:
            continue  # the face without the newest point: the step that added the point has ruled it out
        w = _closest_triangle(a, b, c)
        pt = (w[:, 0, None] * a + w[:, 1, None] * b) + w[:, 2, None] * c
        vv = _dot(pt, pt)
        better = vv < best
        best = np.where(better, vv, best)
        cand = np.zeros((M, 4))
        cand[:, i], cand[:, j], cand[:, k] = w[:, 0], w[:, 1], w[:, 2]
        lam = np.where(better[:, None], cand, lam)
    return lam, inside


def gjk_core_distance(kind_a, h_a, Ra, pa, kind_b, h_b, Rb, pb, tol, max_iter):
    """GJK between the cores of M placed shape pairs of one kind pair: (d_core, pA, pB, status, iterations), the algorithm of
    the module docstring on arrays (every query advances in lockstep; a finished one is left alone)."""
    M = Ra.shape[0]
    v = pa - pb
    flat = (v[:, 0] == 0.0) & (v[:, 1] == 0.0) & (v[:, 2] == 0.0)
    v = np.where(flat[:, None], np.array([1.0, 0.0, 0.0]), v)
    S, A, lam = np.zeros((M, 4, 3)), np.zeros((M, 4, 3)), np.zeros((M, 4))
    n = np.zeros(M, dtype=np.int64)
    status = np.full(M, STATUS_ITERATION_CAP, dtype=np.int32)
    iters = np.zeros(M, dtype=np.int32)
    live = np.arange(M)
    for it in range(1, int(max_iter) + 1):
        if live.size == 0:
            break
        vl = v[live]
        a = _support_world(kind_a, h_a, Ra[live], pa[live], -vl)
        w = a - _support_world(kind_b, h_b, Rb[live], pb[live], vl)
        iters[live] = it
        nl = n[live]
        vn = np.sqrt(_dot(vl, vl))
        sep = _dot(vl, w)
        with np.errstate(divide="ignore", invalid="ignore"):
            done = (nl > 0) & (vn - sep / vn <= tol)
        status[live[done]] = STATUS_OK
        live, a, w, nl, sep = live[~done], a[~done], w[~done], nl[~done], sep[~done]
        if live.size == 0:
            break
        rows = np.arange(live.size)
        Sl, Al = S[live], A[live]
        Sl[rows, nl], Al[rows, nl] = w, a
        nl = nl + 1
        ll = np.zeros((live.size, 4))
        enclosed = np.zeros(live.size, dtype=bool)
        m1, m2, m3, m4 = (nl == k for k in (1, 2, 3, 4))
        ll[m1, 0] = 1.0
        if m2.any():
            ll[m2, :2] = _closest_segment(Sl[m2, 0], Sl[m2, 1])
        if m3.any():
            ll[m3, :3] = _closest_triangle(Sl[m3, 0], Sl[m3, 1], Sl[m3, 2])
        if m4.any():
            ll[m4], enclosed[m4] = _closest_tetrahedron(Sl[m4])
        big = np.zeros(live.size)
        for k in range(4):
            big = np.where(k < nl, np.maximum(big, _dot(Sl[:, k], Sl[:, k])), big)
        keep = (ll > 0.0) & (np.arange(4)[None, :] < nl[:, None])
        order = np.argsort(~keep, axis=1, kind="stable")
        Sl = np.take_along_axis(Sl, order[:, :, None], axis=1)
        Al = np.take_along_axis(Al, order[:, :, None], axis=1)
        ll = np.where(np.take_along_axis(keep, order, axis=1), np.take_along_axis(ll, order, axis=1), 0.0)
        nl = keep.sum(axis=1)
        vl = ((ll[:, 0, None] * Sl[:, 0] + ll[:, 1, None] * Sl[:, 1]) + ll[:, 2, None] * Sl[:, 2]) + ll[:, 3, None] * Sl[:, 3]
        enclosed &= sep <= 0.0  # (a positive lower bound is a separating plane: no flat tetrahedron can talk it away)
        hit = enclosed | (_dot(vl, vl) <= _ZERO_REL_SQ * big)
        S[live], A[live], lam[live], n[live], v[live] = Sl, Al, ll, nl, vl
        status[live[hit]] = STATUS_CORES_INTERSECT
        live = live[~hit]
    pA = ((lam[:, 0, None] * A[:, 0] + lam[:, 1, None] * A[:, 1]) + lam[:, 2, None] * A[:, 2]) + lam[:, 3, None] * A[:, 3]
    cut = status == STATUS_CORES_INTERSECT
    pB = np.where(cut[:, None], pA, pA - v)
    diff = pA - pB
    d_core = np.sqrt(_dot(diff, diff))
    return d_core, pA, pB, status, iters


def geometry_placements(model, geom_model, q):
    """[(R (N, 3, 3), p (N, 3)), ...]: oM_parent . placement of every geometry object at the (N, nq) configurations q, through
    the forward kinematics of the calibration mirror."""
    from ..calibration.calibration_tools import _as_configurations, _mul, _se3_tuple, _world_placements
    q = _as_configurations(model, q)
    objs = geom_model.geometryObjects
    for o in objs:
        if not 0 <= o.parentJoint < model.njoints:
            raise ValueError("geometry %r sits on joint %d, the model has %d" % (o.name, o.parentJoint, model.njoints))
    oM = _world_placements(model, q, [o.parentJoint for o in objs])
    out = []
    for o in objs:
        R, p = _mul(oM[o.parentJoint][1], _se3_tuple(o.placement))
        out.append((np.broadcast_to(R, (q.shape[0], 3, 3)), np.broadcast_to(p, (q.shape[0], 3))))
    return out


def collision_distances_mirror(model, geom_model, q, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER):
    """``(d, pA, pB, status, iterations)`` of every collision pair at the (N, nq) configurations ``q``: d (N, n_pairs), the
    witness points (N, n_pairs, 3) in the world frame on the cores, status and iteration counts (N, n_pairs) int32 -- the
    NumPy statement of ``figh_collision_distances`` (module docstring), the route taken without a device."""
    if not tol > 0.0 or not 1 <= int(max_iter) <= 1024:
        raise ValueError("tol must be positive and max_iter in [1, 1024]")
    placed = geometry_placements(model, geom_model, q)
    N = placed[0][0].shape[0] if placed else np.atleast_2d(np.asarray(q)).shape[0]
    P = len(geom_model.collisionPairs)
    d, pA, pB = np.zeros((N, P)), np.zeros((N, P, 3)), np.zeros((N, P, 3))
    status, iters = np.zeros((N, P), dtype=np.int32), np.zeros((N, P), dtype=np.int32)
    for k, pair in enumerate(geom_model.collisionPairs):
        ga, gb = geom_model.geometryObjects[pair.first].geometry, geom_model.geometryObjects[pair.second].geometry
        (Ra, pa), (Rb, pb) = placed[pair.first], placed[pair.second]
        core, pA[:, k], pB[:, k], status[:, k], iters[:, k] = gjk_core_distance(
            ga.kind, core_half_extents(ga.kind, ga.dimensions), Ra, pa, gb.kind, core_half_extents(gb.kind, gb.dimensions),
            Rb, pb, float(tol), int(max_iter))
        d[:, k] = core - (ga.core_radius + gb.core_radius)
    return d, pA, pB, status, iters


# -------------------------------------------------------------------------------------------------------------- device
def collision_distances_device(robot, geom_model, q_ptr, ldq, B, n_per, idx, out_ptr, ld_b, tol=DEFAULT_TOL,
                               max_iter=DEFAULT_MAX_ITER, witness_ptr=None, status_ptr=None):
    """``figh_collision_distances`` for a geometry model: out[b ld_b + i n_pairs + p] for the samples ``idx`` (None: every
    sample) of B trajectories of n_per configurations behind the device address ``q_ptr``."""
    from .. import _lib
    kind, parent, placement, dims, pairs, _ = geometry_table(geom_model)
    _lib.collision_distances(robot.device_model(), B, n_per, idx, q_ptr, ldq, kind, parent, placement, dims, pairs, tol,
                             max_iter, out_ptr, ld_b, witness_ptr, status_ptr)


def _have_device():
    from .. import _lib
    return _lib.device_count() > 0


class CollisionWrapper:
    """``CollisionWrapper(robot, geom_model=None, geom_data=None, viz=None)`` of robotcollisions.py:20-134.
    ``computeCollisions`` takes one configuration, an (N, nq) array or a ``GpuMatrix`` of configurations; the distances come
    from ``figh_collision_distances`` when a device is there (always for a ``GpuMatrix``), from the NumPy mirror otherwise;
    ``use_device=False`` takes the mirror for host arrays whatever the machine has."""

    def __init__(self, robot, geom_model=None, geom_data=None, viz=None, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER,
                 use_device=None):
        self.robot, self.viz = robot, viz
        self.rmodel = robot.model
        self.rdata = robot.data
        self.gmodel = robot.geom_model if geom_model is None else geom_model
        self.gdata = geom_data
        self.tol, self.max_iter, self.use_device = float(tol), int(max_iter), use_device
        self._d = self._status = None
        self._single = True

    def add_collisions(self):
        self.gmodel.addAllCollisionPairs()

    def remove_collisions(self, srdf_model_path):
        if srdf_model_path is None:
            return
        raise NotImplementedError("SRDF parsing is not part of this package: drop pairs from gmodel.collisionPairs directly")

    def computeCollisions(self, q, geom_data=None):
        """True when some pair is in collision (d <= 0); per row, a bool array, for a batch of configurations."""
        from ..device import GpuMatrix
        n_pairs = len(self.gmodel.collisionPairs)
        if isinstance(q, GpuMatrix):
            self._single = False
            self._d, self._status = self._on_device(q.ptr, q.ld, q.rows)
        else:
            qa = np.asarray(q, dtype=np.float64)
            self._single = qa.ndim == 1
            qa = np.ascontiguousarray(qa.reshape(1, -1) if self._single else qa)
            if qa.ndim != 2 or qa.shape[1] != self.rmodel.nq:
                raise ValueError("expected (N, %d) configurations, got shape %r" % (self.rmodel.nq, qa.shape))
            if n_pairs and (_have_device() if self.use_device is None else self.use_device):
                from .. import _lib
                d_q = _lib.DeviceArray.from_host(qa.reshape(-1))
                self._d, self._status = self._on_device(d_q.ptr, qa.shape[1], qa.shape[0])
            else:
                self._d, _, _, self._status, _ = collision_distances_mirror(self.rmodel, self.gmodel, qa, self.tol,
                                                                            self.max_iter)
        hit = np.any(self._d <= 0.0, axis=1)
        return bool(hit[0]) if self._single else hit

    def _on_device(self, q_ptr, ldq, N):
        from .. import _lib
        n_pairs = len(self.gmodel.collisionPairs)
        if n_pairs == 0:
            return np.zeros((N, 0)), np.zeros((N, 0), dtype=np.int32)
        out = _lib.DeviceArray((N * n_pairs,), np.float64)
        st = _lib.DeviceArray((N * n_pairs,), np.int32)
        collision_distances_device(self.robot, self.gmodel, q_ptr, ldq, 1, N, None, out.ptr, N * n_pairs, self.tol,
                                   self.max_iter, None, st.ptr)
        return out.to_host().reshape(N, n_pairs), (st.to_host() & 0xFFFF).reshape(N, n_pairs)

    def _results(self):
        if self._d is None:
            raise RuntimeError("computeCollisions(q) has not been called")
        return self._d

    def getDistances(self):
        """(n_pairs,) for one configuration, (N, n_pairs) for a batch: the distance of every pair, in pair order."""
        d = self._results()
        return d[0].copy() if self._single else d.copy()

    def getStatus(self):
        """The status of every query (``STATUS_OK`` / ``STATUS_CORES_INTERSECT`` / ``STATUS_ITERATION_CAP``), shaped like
        ``getDistances()``."""
        self._results()
        return self._status[0].copy() if self._single else self._status.copy()

    def getCollisionList(self, row=0):
        """Triplets [index, gmodel.collisionPairs[index], distance] of the pairs in collision (d <= 0) at configuration
        ``row`` of the last ``computeCollisions``."""
        d = self._results()[row]
        return [[k, self.gmodel.collisionPairs[k], float(d[k])] for k in range(len(d)) if d[k] <= 0.0]

    def getCollisionDistances(self, collisions=None):
        if collisions is None:
            collisions = self.getCollisionList()
        if len(collisions) == 0:
            return np.array([])
        return np.array([self._results()[0][i] if self._single else r for (i, c, r) in collisions])

    def getAllpairs(self):
        d = self._results()[0]
        for k, cp in enumerate(self.gmodel.collisionPairs):
            print("collision pair:", k, " ", self.gmodel.geometryObjects[cp.first].name, ",",
                  self.gmodel.geometryObjects[cp.second].name, "- collision:", "Yes" if d[k] <= 0.0 else "No")

    def check_collision(self, q=None):
        """True when a pair of the last ``computeCollisions`` is in collision (the reference ignores ``q`` too)."""
        return bool(np.any(self._results() <= 0.0))

    # --- display: not mirrored
    def _no_display(self, *args, **kwargs):
        raise NotImplementedError("display needs a Meshcat viewer, which this package does not wrap")

    initDisplay = createDisplayPatchs = displayContact = displayCollisions = _no_display
