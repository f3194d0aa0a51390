"""An independent reference for XPBD joint projection: prepare, solve, velocity projection, joint damping, forces.

Plain numpy, generic over the scalar type (np.float32, np.float64, np.longdouble).  Written from the reference project's text
(src/dynamics/solver/xpbd/{mod, plugin, positional_constraint, angular_constraint}.rs, xpbd/joints/*.rs, xpbd/joints/shared/*.rs,
dynamics/joints/mod.rs:310-474, solver/plugin.rs:759-806, solver_body/mod.rs:429-513) and from Müller et al. 2020, "Detailed Rigid Body Simulation
with Extended Position Based Dynamics", without reading the kernels or the oracle.  It is NOT a transliteration: wherever exact arithmetic makes two
forms equal it takes the other one, so that a formula the kernel and the oracle share is checked against something that does not share it.

  * vectors are rotated by 3x3 matrices, never by a quaternion sandwich.  `Quat * Vec3` of glam is v (w w - b.b) + 2 b (v.b) + 2 w (b x v); the matrix
    (w w - b.b) I + 2 b b^T + 2 w [b]x is the same map for ANY quaternion, unit or not (delta rotations are never renormalised inside a substep);
  * a limit angle is atan2(s, +-sqrt(1 - s^2)) with s = (n1 x n2).n and the sign of n1.n2, not asin with the obtuse fix-up.  For unit n1, n2
    perpendicular to n (the swing and twist constructions) this is atan2((n1 x n2).n, n1.n2); the revolute joint hands over b2 of body 2, which
    leaves the plane perpendicular to a1 as soon as the hinge axes are misaligned, and there the reference's own definition (asin of the triple product)
    is what the form above equals and the plain atan2 does not;
  * the prismatic correction off the axis is minus the component of the separation perpendicular to the free axis u, times |e|^2 where
    e = any_orthogonal_vector(u) = (|x| > |y|) ? (-z, 0, x) : (0, z, -y).  The reference sums two zero limits along e and u x e, and glam does not
    normalise e: for an axis-aligned u the factor is 1, for any other it is 1 - min(x^2, y^2).  That is the reference's definition and it is kept;
  * the limit rotation is Rodrigues' matrix; sin and cos are numpy's.

What follows the reference's own choices: the rotation update of a positional impulse (angle |v| about v = I^-1 (r x p), left-multiplied), `max_element`
of the effective inverse mass in w, delta-lambda = (-c - a~ lambda) / (w1 + w2 + a~) with lambda = 0 and 0 when w1 + w2 <= eps, the fixed-angle error
-2 vec(D dq1 dq2^-1), glam's any_orthonormal_vector, Matrix::from_quat in the spherical prepare, the twist max_correction switch at a1.a2 > -0.5, DUMMY
sides (no SolverBody, dominance), unprepared joints that are still solved, totals cleared at prepare and accumulated over substeps,
force = total * substeps / dt^2, the shared mutable DUMMY bodies of joint_damping::<T>.

Conditioning: every solve appends, per joint, its distance to each discontinuity it passed (`report`), see `MARGIN_KEYS`.

MUTATIONS are deliberate errors for the negative controls of tests/test_joint_projection_cpu.py.
"""
import numpy as np

FIXED, REVOLUTE, SPHERICAL, PRISMATIC, DISTANCE = 0, 1, 2, 3, 4
HAS_LIMIT1, HAS_LIMIT2 = 1, 2
NO_SOLVER_BODY = 1 << 31
IS_KINEMATIC = 1 << 6
LOCK_TX, LOCK_TY, LOCK_TZ = 0b100000, 0b010000, 0b001000
DUMMY_DOMINANCE = 128   # i8::MAX as i16 + 1

MUTATIONS = ("limit_sign", "no_obtuse_branch", "limit_compliances_swapped", "inv_mass_x", "no_twist_switch", "body2_not_negated", "force_without_substeps")

# distance to: the +-pi wrap of a limit angle [rad]; |s| = 1 where asin / sqrt(1 - s^2) lose their derivative (0 exactly is a clean 90 degrees);
# the -0.5 twist switch; the sign of z and the |x| = |y| switch of the orthogonal-vector constructions; lengths that are divided by; w1 + w2 above eps
MARGIN_KEYS = ("wrap", "asin", "twist_switch", "ortho_z", "ortho_xy", "length", "w_sum")


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def norm(a):
    return np.sqrt(a @ a)


def skew(b):
    z = b.dtype.type(0)
    return np.array([[z, -b[2], b[1]], [b[2], z, -b[0]], [-b[1], b[0], z]], b.dtype)


def quat_matrix(q):
    """The linear map of glam's `Quat * Vec3` as a matrix, valid for a quaternion of any length."""
    b, w = q[:3], q[3]
    return (w * w - b @ b) * np.eye(3, dtype=q.dtype) + 2 * np.outer(b, b) + (2 * w) * skew(b)


def mat3_from_quat(q):
    """glam Mat3::from_quat (the spherical prepare)."""
    x, y, z, w = q
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz, yy, yz, zz, wx, wy, wz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2, w * x2, w * y2, w * z2
    one = q.dtype.type(1)
    return np.array([[one - (yy + zz), xy - wz, xz + wy], [xy + wz, one - (xx + zz), yz - wx], [xz - wy, yz + wx, one - (xx + yy)]], q.dtype)


def qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], a.dtype)


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], q.dtype)


def rotation_about(v):
    """The quaternion of the rotation of angle |v| about v (Quaternion::from_scaled_axis)."""
    T = v.dtype.type
    angle = norm(v)
    if angle == 0:
        return np.array([0, 0, 0, 1], v.dtype)
    half = angle * T(0.5)
    return np.concatenate([v / angle * np.sin(half), [np.cos(half)]]).astype(v.dtype)


def rodrigues(n, phi):
    c, s = np.cos(phi), np.sin(phi)
    return c * np.eye(3, dtype=n.dtype) + s * skew(n) + (n.dtype.type(1) - c) * np.outer(n, n)


def any_orthonormal_vector(v):
    T = v.dtype.type
    sign = T(-1) if np.signbit(v[2]) else T(1)
    a = T(-1) / (sign + v[2])
    b = v[0] * v[1] * a
    return np.array([b, sign + v[1] * v[1] * a, -v[1]], v.dtype)


def sym(m6):
    m00, m01, m02, m11, m12, m22 = m6
    return np.array([[m00, m01, m02], [m01, m11, m12], [m02, m12, m22]], m6.dtype)


class JointReference:
    """`joints`: the avn_joints arrays, `poses`: position / rotation / center_of_mass / body_flags of the uploaded bodies -- both as the world holds them
    (rounded to the world's scalar type by the caller).  `h`, `dt`: the substep's and the step's delta seconds as the world's type has them."""

    def __init__(self, T, joints, poses, h, dt, substeps, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.T, self.mut = T, mutation
        self.eps = T(np.finfo(T).eps)
        self.pi = T(np.pi) if T is not np.longdouble else np.arctan2(T(0), T(-1))
        self.h, self.dt, self.substeps = T(h), T(dt), int(substeps)
        f = lambda k, shape: np.asarray(joints[k]).astype(T).reshape(shape) if joints.get(k) is not None else None
        J = self.J = len(joints["body1"])
        self.type = np.asarray(joints["joint_type"]).astype(int)
        self.b1, self.b2 = np.asarray(joints["body1"]).astype(int), np.asarray(joints["body2"]).astype(int)
        self.anchor1, self.anchor2 = f("local_anchor1", (J, 3)), f("local_anchor2", (J, 3))
        ident = np.tile(np.array([0, 0, 0, 1], T), (J, 1))
        self.basis1 = f("local_basis1", (J, 4)) if joints.get("local_basis1") is not None else ident
        self.basis2 = f("local_basis2", (J, 4)) if joints.get("local_basis2") is not None else ident
        self.axis = f("axis", (J, 3)) if joints.get("axis") is not None else np.zeros((J, 3), T)
        zeros = np.zeros(J, T)
        self.lim = [(f(a, (J,)) if joints.get(a) is not None else zeros, f(b, (J,)) if joints.get(b) is not None else zeros)
                    for a, b in (("limit_min", "limit_max"), ("limit2_min", "limit2_max"))]
        self.limit_flags = np.asarray(joints["limit_flags"]).astype(int) if joints.get("limit_flags") is not None else np.zeros(J, int)
        self.compliance = f("compliance", (J, 3))
        self.damped = joints.get("damping_linear") is not None and joints.get("damping_angular") is not None
        self.damping = (f("damping_linear", (J,)), f("damping_angular", (J,))) if self.damped else None
        self.pos = np.asarray(poses["position"]).astype(T)
        self.rot = np.asarray(poses["rotation"]).astype(T)
        n = len(self.pos)
        self.com = np.asarray(poses["center_of_mass"]).astype(T) if poses.get("center_of_mass") is not None else np.zeros((n, 3), T)
        self.disabled = (np.asarray(poses["body_flags"]).astype(int) & 2) != 0 if poses.get("body_flags") is not None else np.zeros(n, bool)
        self.order = [j for t in (FIXED, REVOLUTE, SPHERICAL, PRISMATIC, DISTANCE) for j in range(J) if self.type[j] == t]
        z3 = lambda: np.zeros((J, 3), T)
        # solver data: the components' Default until a prepare fills them
        self.world_r1, self.world_r2, self.center_difference = z3(), z3(), z3()
        self.vec = {k: z3() for k in ("a1", "a2", "b1", "b2")}   # revolute a / b axes, spherical swing (a) / twist (b) axes, prismatic free axis (a1)
        self.D = ident.copy()
        self.total_lagrange, self.total_rot = z3(), [z3(), z3()]
        self.report = []

    # ---- prepare_xpbd_joint ---------------------------------------------------------------------------------------------------------------------
    def prepare(self):
        self.total_lagrange[:] = 0; self.total_rot[0][:] = 0; self.total_rot[1][:] = 0
        for j in self.order:
            i1, i2 = self.b1[j], self.b2[j]
            if self.disabled[i1] or self.disabled[i2]:
                continue
            t = self.type[j]
            q1, q2 = self.rot[i1], self.rot[i2]
            R1, R2 = (mat3_from_quat(q1), mat3_from_quat(q2)) if t == SPHERICAL else (quat_matrix(q1), quat_matrix(q2))
            S1, S2 = quat_matrix(q1), quat_matrix(q2)
            self.world_r1[j] = R1 @ (self.anchor1[j] - self.com[i1])
            self.world_r2[j] = R2 @ (self.anchor2[j] - self.com[i2])
            self.center_difference[j] = (self.pos[i2] - self.pos[i1]) + (S2 @ self.com[i2] - S1 @ self.com[i1])
            B1, B2 = quat_matrix(self.basis1[j]), quat_matrix(self.basis2[j])
            if t in (FIXED, PRISMATIC):
                self.D[j] = qmul(qmul(q1, self.basis1[j]), qconj(qmul(q2, self.basis2[j])))
            if t == PRISMATIC:
                self.vec["a1"][j] = quat_matrix(qmul(q1, self.basis1[j])) @ self.axis[j]
            if t == REVOLUTE:
                F1, F2 = quat_matrix(qmul(q1, self.basis1[j])), quat_matrix(qmul(q2, self.basis2[j]))
                o = any_orthonormal_vector(self.axis[j])
                self.vec["a1"][j], self.vec["a2"][j], self.vec["b1"][j], self.vec["b2"][j] = F1 @ self.axis[j], F2 @ self.axis[j], F1 @ o, F2 @ o
            if t == SPHERICAL:
                o = any_orthonormal_vector(self.axis[j])
                self.vec["a1"][j], self.vec["a2"][j] = R1 @ (B1 @ o), R2 @ (B2 @ o)
                self.vec["b1"][j], self.vec["b2"][j] = R1 @ (B1 @ self.axis[j]), R2 @ (B2 @ self.axis[j])

    def ortho_z_margin(self, j):
        """The sign(z) switch of any_orthonormal_vector matters for the types that call it on the joint's axis."""
        return abs(float(self.axis[j][2])) if self.type[j] in (REVOLUTE, SPHERICAL) else np.inf

    # ---- solve_xpbd_joint -----------------------------------------------------------------------------------------------------------------------
    def _sides(self, sb, j):
        T = self.T
        out = []
        has = [not (int(sb["flags"][i]) & NO_SOLVER_BODY) for i in (self.b1[j], self.b2[j])]
        dom = [int(sb["dominance"][i]) if ok else DUMMY_DOMINANCE for i, ok in zip((self.b1[j], self.b2[j]), has)]
        rel = dom[0] - dom[1]
        for side, i in enumerate((self.b1[j], self.b2[j])):
            dummy_inertia = (not has[side]) or (rel > 0 if side == 0 else rel < 0)
            if dummy_inertia:
                im, I = np.zeros(3, T), np.zeros((3, 3), T)
            else:
                m, fl = T(sb["inv_mass"][i]), int(sb["flags"][i])
                im = np.array([0 if fl & LOCK_TX else m, 0 if fl & LOCK_TY else m, 0 if fl & LOCK_TZ else m], T)
                I = sym(np.asarray(sb["inv_inertia_world"][i]).astype(T))
            if has[side]:
                dp, dq = self.dp[i].copy(), self.dq[i].copy()
            else:
                dp, dq = np.zeros(3, T), np.array([0, 0, 0, 1], T)
            out.append(dict(i=i, has=has[side], dp=dp, dq=dq, im=im, I=I))
        return out

    def _lagrange(self, c, w_sum, compliance, m):
        m["w_sum"] = min(m["w_sum"], abs(float(w_sum) - float(self.eps)) if w_sum > 0 else np.inf)   # (w = 0: a pair that cannot move, far from any switch)
        if w_sum <= self.eps:
            return self.T(0)
        tilde = compliance / (self.h * self.h)
        return -c / (w_sum + tilde)

    def _inv_mass_scalar(self, im):
        return im[0] if self.mut == "inv_mass_x" else im.max()

    def _positional(self, s1, s2, p, r1, r2):
        p2 = p if self.mut == "body2_not_negated" else -p
        s1["dp"] = s1["dp"] + p * s1["im"]
        s1["dq"] = qmul(rotation_about(s1["I"] @ cross(r1, p)), s1["dq"])
        s2["dp"] = s2["dp"] + p2 * s2["im"]
        s2["dq"] = qmul(rotation_about(s2["I"] @ cross(r2, p2)), s2["dq"])

    def _separation(self, s1, s2, j):
        r1, r2 = quat_matrix(s1["dq"]) @ self.world_r1[j], quat_matrix(s2["dq"]) @ self.world_r2[j]
        return r1, r2, (s2["dp"] - s1["dp"]) + (r2 - r1) + self.center_difference[j]

    def _w_pos(self, s, r, n):
        rn = cross(r, n)
        return self._inv_mass_scalar(s["im"]) + rn @ (s["I"] @ rn)

    def _point(self, s1, s2, j, compliance, m):
        r1, r2, sep = self._separation(s1, s2, j)
        mag2 = sep @ sep
        if mag2 == 0:
            return
        mag = np.sqrt(mag2)
        n = -sep / mag
        dl = self._lagrange(mag, self._w_pos(s1, r1, n) + self._w_pos(s2, r2, n), compliance, m)
        p = dl * n
        self.total_lagrange[j] += p
        self._positional(s1, s2, p, r1, r2)

    def _align(self, s1, s2, difference, compliance, m):
        """AngularConstraint::align_orientation: returns delta-lambda * axis."""
        angle = norm(difference)
        if angle <= self.eps:
            return np.zeros(3, self.T)
        axis = difference / angle
        dl = self._lagrange(angle, axis @ (s1["I"] @ axis) + axis @ (s2["I"] @ axis), compliance, m)
        if abs(dl) > self.eps:
            p = -dl * axis
            p2 = p if self.mut == "body2_not_negated" else -p
            s1["dq"] = qmul(rotation_about(s1["I"] @ p), s1["dq"])
            s2["dq"] = qmul(rotation_about(s2["I"] @ p2), s2["dq"])
        return dl * axis

    def _limit_correction(self, lo, hi, n, n1, n2, max_correction, m, tag):
        T = self.T
        s, c = cross(n1, n2) @ n, n1 @ n2
        root = np.sqrt(max(T(1) - s * s, T(0)))
        phi = np.arctan2(s, -root if (c < 0 and self.mut != "no_obtuse_branch") else root)
        m["wrap"] = min(m["wrap"], float(self.pi) - abs(float(phi)))
        m["asin"] = min(m["asin"], 1.0 - abs(float(s)) if abs(s) != 1 else np.inf)
        m[tag + "_phi"] = float(phi); m[tag + "_cos"] = float(c)
        if not (phi < lo or phi > hi):
            return None
        phi = min(max(phi, lo), hi)
        corr = cross(rodrigues(n, phi) @ n1, n2)
        if self.mut == "limit_sign":
            corr = -corr
        l2 = corr @ corr
        if l2 > max_correction * max_correction:
            corr = max_correction * (corr / np.sqrt(l2))
        return corr

    def _fixed_angle(self, s1, s2, j, compliance, m):
        q = qmul(qmul(self.D[j], s1["dq"]), qconj(s2["dq"]))
        self.total_rot[0][j] += self._align(s1, s2, self.T(-2) * q[:3], compliance, m)

    def solve(self, sb):
        """One XPBD_SOLVE from the world's SolverBody state `sb` (a solver_bodies_download): returns (delta_position, delta_rotation) after it."""
        T = self.T
        self.dp = np.asarray(sb["delta_position"]).astype(T)
        self.dq = np.asarray(sb["delta_rotation"]).astype(T)
        report = {}
        for j in self.order:
            s1, s2 = self._sides(sb, j)
            start = [(s["dp"], s["dq"]) for s in (s1, s2)]
            t = self.type[j]
            k = self.compliance[j]
            if self.mut == "limit_compliances_swapped":
                k = k[[0, 2, 1]]
            lim1, lim2 = self.limit_flags[j] & HAS_LIMIT1, self.limit_flags[j] & HAS_LIMIT2
            m = {key: np.inf for key in MARGIN_KEYS}
            m["ortho_z"] = self.ortho_z_margin(j)
            if t == FIXED:
                self._fixed_angle(s1, s2, j, k[1], m)
                self._point(s1, s2, j, k[0], m)
            elif t == REVOLUTE:
                a1, a2 = quat_matrix(s1["dq"]) @ self.vec["a1"][j], quat_matrix(s2["dq"]) @ self.vec["a2"][j]
                self.total_rot[0][j] += self._align(s1, s2, cross(a1, a2), k[1], m)
                if lim1:
                    M1, M2 = quat_matrix(s1["dq"]), quat_matrix(s2["dq"])
                    corr = self._limit_correction(self.lim[0][0][j], self.lim[0][1][j], M1 @ self.vec["a1"][j], M1 @ self.vec["b1"][j], M2 @ self.vec["b2"][j], self.pi, m, "l1")
                    if corr is not None:
                        self.total_rot[1][j] += self._align(s1, s2, corr, k[2], m)
                self._point(s1, s2, j, k[0], m)
            elif t == SPHERICAL:
                self._point(s1, s2, j, k[0], m)
                if lim1:
                    a1, a2 = quat_matrix(s1["dq"]) @ self.vec["a1"][j], quat_matrix(s2["dq"]) @ self.vec["a2"][j]
                    n = cross(a1, a2)
                    length = norm(n)
                    m["length"] = min(m["length"], float(length))
                    if length > self.eps:
                        corr = self._limit_correction(self.lim[0][0][j], self.lim[0][1][j], n / length, a1, a2, self.pi, m, "l1")
                        if corr is not None:
                            self.total_rot[0][j] += self._align(s1, s2, corr, k[1], m)
                if lim2:
                    M1, M2 = quat_matrix(s1["dq"]), quat_matrix(s2["dq"])
                    a1, a2 = M1 @ self.vec["a1"][j], M2 @ self.vec["a2"][j]
                    n = a1 + a2
                    length = norm(n)
                    m["length"] = min(m["length"], float(length))
                    if length > self.eps:
                        n = n / length
                        b1, b2 = M1 @ self.vec["b1"][j], M2 @ self.vec["b2"][j]
                        n1, n2 = b1 - (n @ b1) * n, b2 - (n @ b2) * n
                        l1, l2 = norm(n1), norm(n2)
                        m["length"] = min(m["length"], float(l1), float(l2))
                        if l1 > self.eps and l2 > self.eps:
                            d = a1 @ a2
                            m["twist_switch"] = abs(float(d) + 0.5); m["swing_cos"] = float(d)
                            max_correction = 2 * self.pi if (d > T(-0.5) or self.mut == "no_twist_switch") else self.h
                            corr = self._limit_correction(self.lim[1][0][j], self.lim[1][1][j], n, n1 / l1, n2 / l2, max_correction, m, "l2")
                            if corr is not None:
                                self.total_rot[1][j] += self._align(s1, s2, corr, k[2], m)
            elif t == PRISMATIC:
                self._fixed_angle(s1, s2, j, k[1], m)
                r1, r2, sep = self._separation(s1, s2, j)
                u = quat_matrix(s1["dq"]) @ self.vec["a1"][j]
                m["ortho_xy"] = abs(abs(float(u[0])) - abs(float(u[1])))
                along = sep @ u
                m["along"] = float(along)
                dx = np.zeros(3, T)
                if lim1:
                    lo, hi = self.lim[0][0][j], self.lim[0][1][j]
                    if along < lo: dx = dx + u * (lo - along)
                    elif along > hi: dx = dx - u * (along - hi)
                e2 = (u[2] * u[2] + u[0] * u[0]) if abs(u[0]) > abs(u[1]) else (u[2] * u[2] + u[1] * u[1])
                dx = dx - e2 * (sep - along * u)
                mag = norm(dx)
                m["length"] = min(m["length"], float(mag))
                if mag > self.eps:
                    n = dx / mag
                    dl = self._lagrange(mag, self._w_pos(s1, r1, n) + self._w_pos(s2, r2, n), k[0], m)
                    p = dl * n
                    self.total_lagrange[j] += p
                    self._positional(s1, s2, p, r1, r2)
            elif t == DISTANCE:
                r1, r2, sep = self._separation(s1, s2, j)
                d2 = sep @ sep
                if d2 > self.eps:
                    d = np.sqrt(d2)
                    m["length"] = min(m["length"], float(d)); m["distance"] = float(d)
                    lo, hi = self.lim[0][0][j], self.lim[0][1][j]
                    n, c = (sep / d, lo - d) if d < lo else ((-sep / d, d - hi) if d > hi else (None, T(0)))
                    if n is not None and c > self.eps:
                        dl = self._lagrange(c, self._w_pos(s1, r1, n) + self._w_pos(s2, r2, n), k[0], m)
                        p = dl * n
                        self.total_lagrange[j] += p
                        self._positional(s1, s2, p, r1, r2)
            for s in (s1, s2):
                if s["has"]:
                    self.dp[s["i"]], self.dq[s["i"]] = s["dp"], s["dq"]
            m["correction"] = max(float(np.abs(s[key] - b).max()) for s, before in zip((s1, s2), start) for key, b in zip(("dp", "dq"), before))
            report[j] = m
        self.report.append(report)
        return self.dp.copy(), self.dq.copy()

    # ---- project_linear_velocity, project_angular_velocity (xpbd/plugin.rs:191-240) ---------------------------------------------------------------------
    def project_velocities(self, sb, pre):
        """`sb`: the state after XPBD_SOLVE, `pre`: the state before it (PreSolveDeltaPosition / PreSolveDeltaRotation)."""
        T = self.T
        lin, ang = np.asarray(sb["linear_velocity"]).astype(T), np.asarray(sb["angular_velocity"]).astype(T)
        dp, dq = np.asarray(sb["delta_position"]).astype(T), np.asarray(sb["delta_rotation"]).astype(T)
        dp0, dq0 = np.asarray(pre["delta_position"]).astype(T), np.asarray(pre["delta_rotation"]).astype(T)
        for i in range(len(lin)):
            if int(sb["flags"][i]) & NO_SOLVER_BODY:
                continue
            lin[i] += (dp[i] - dp0[i]) / self.h
            d = qmul(dq[i], qconj(dq0[i]))
            w = T(2) * d[:3] / self.h
            ang[i] += -w if d[3] < 0 else w
        return lin, ang

    # ---- joint_damping::<T> (solver/plugin.rs:759-806) --------------------------------------------------------------------------------------------------
    def damp(self, sb):
        T = self.T
        lin, ang = np.asarray(sb["linear_velocity"]).astype(T), np.asarray(sb["angular_velocity"]).astype(T)
        if not self.damped:
            return lin, ang
        one = T(1)
        for t in (FIXED, REVOLUTE, SPHERICAL, PRISMATIC, DISTANCE):
            dummy = [dict(lin=np.zeros(3, T), ang=np.zeros(3, T)), dict(lin=np.zeros(3, T), ang=np.zeros(3, T))]   # one mutable pair per system
            for j in (j for j in self.order if self.type[j] == t):
                side = []
                for k, i in enumerate((self.b1[j], self.b2[j])):
                    fl = int(sb["flags"][i])
                    if fl & NO_SOLVER_BODY:
                        side.append((None, dummy[k], np.zeros(3, T), False))
                    else:
                        m = T(sb["inv_mass"][i])
                        im = np.array([0 if fl & LOCK_TX else m, 0 if fl & LOCK_TY else m, 0 if fl & LOCK_TZ else m], T)
                        side.append((i, dict(lin=lin[i].copy(), ang=ang[i].copy()), im, bool(fl & IS_KINEMATIC)))
                (i1, v1, w1, kin1), (i2, v2, w2, kin2) = side
                d_omega = (v2["ang"] - v1["ang"]) * min(self.damping[1][j] * self.h, one)
                if not kin1: v1["ang"] = v1["ang"] + d_omega
                if not kin2: v2["ang"] = v2["ang"] - d_omega
                d_v = (v2["lin"] - v1["lin"]) * min(self.damping[0][j] * self.h, one)
                ws = w1 + w2
                with np.errstate(divide="ignore"):
                    rec = np.where((ws != 0) & np.isfinite(ws), one / np.where(ws != 0, ws, one), T(0)).astype(T)
                p = d_v * rec
                v1["lin"] = v1["lin"] + p * w1
                v2["lin"] = v2["lin"] - p * w2
                for i, v in ((i1, v1), (i2, v2)):
                    if i is not None:
                        lin[i], ang[i] = v["lin"], v["ang"]
        return lin, ang

    # ---- writeback_joint_forces (xpbd/plugin.rs:242-260) ------------------------------------------------------------------------------------------------
    def forces(self):
        d2 = self.dt * self.dt
        rhs = (self.T(1) / d2 if (d2 != 0 and np.isfinite(d2)) else self.T(0))
        if self.mut != "force_without_substeps":
            rhs = rhs * self.T(self.substeps)
        return self.total_lagrange * rhs, (self.total_rot[0] + self.total_rot[1]) * rhs

    def total_rotation_lagrange(self):
        return self.total_rot[0] + self.total_rot[1]
