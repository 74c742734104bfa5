"""The configuration integrator q (+) v in 50-digit arithmetic (mpmath), for the tests that pin pose_numpy.integrate (on the CPU) and
the device's integrate kernel (on the GPU) to the group exponentials themselves: SE(3) for the free-flyer, SO(3) for the spherical
joint, SE(2) for the planar joint, SO(2) on (cos, sin) for the unbounded revolute joints, a plain sum for every other coordinate;
a composite integrates sub-joint by sub-joint.  Conventions are pinocchio's: twists [linear; angular] in the joint's own frame,
quaternions (x, y, z, w), the free-flyer's quaternion kept in the hemisphere of the one it came from, the spherical joint's the
plain product; a quaternion or (cos, sin) pair stands for the rotation of its direction and is returned on the unit sphere.
No thresholds: every coefficient is written so that 50 digits hold at every angle (sin^2 of the half angle for 1 - cos, the
Maclaurin series for (th - sin th) / th^3 below th = 0.1), and th = 0 takes the limits.  The inputs are taken as the exact doubles
they are; the result is rounded to double once, at the end.  A sum of two doubles rounded once is what numpy's `+` returns, so
the plain sums are left to it."""
import numpy as np
from mpmath import mp, mpf

from loik_amd import workloads as W
from pose_numpy import J_FREEFLYER, J_PLANAR, J_RUBU, J_RUBX, J_RUBY, J_RUBZ, J_SPHERICAL

DIGITS = 50


def _vec(x):
    return [mpf(float(t)) for t in x]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
            a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def _rotate(qt, p):
    """R(qt / |qt|) p"""
    n = mp.sqrt(sum(c * c for c in qt))
    x, y, z, w = (c / n for c in qt)
    u = [x, y, z]
    t = [2 * c for c in _cross(u, p)]
    ut = _cross(u, t)
    return [p[k] + w * t[k] + ut[k] for k in range(3)]


def _unit(qt):
    n = mp.sqrt(sum(c * c for c in qt))
    return [c / n for c in qt]


def exp_quat(w):
    """the quaternion of exp([w]x)"""
    th = mp.sqrt(sum(c * c for c in w))
    k = mpf(1) / 2 if th == 0 else mp.sin(th / 2) / th
    return [k * w[0], k * w[1], k * w[2], mp.cos(th / 2)]


def se3_coefficients(th):
    """(a, b) = ((1 - cos th) / th^2, (th - sin th) / th^3)"""
    if th == 0:
        return mpf(1) / 2, mpf(1) / 6
    a = 2 * (mp.sin(th / 2) / th) ** 2
    if th < mpf("0.1"):
        t2, b, term, k = th * th, mpf(0), mpf(1) / 6, 0
        while abs(term) > mpf(10) ** (-DIGITS - 10):
            b += term
            term *= -t2 / ((2 * k + 4) * (2 * k + 5))
            k += 1
        return a, b
    return a, (th - mp.sin(th)) / th ** 3


def se3(q7, v6):
    t, qt, vl, w = _vec(q7[:3]), _vec(q7[3:7]), _vec(v6[:3]), _vec(v6[3:6])
    a, b = se3_coefficients(mp.sqrt(sum(c * c for c in w)))
    wxv = _cross(w, vl)
    wwv = _cross(w, wxv)
    p = _rotate(qt, [vl[k] + a * wxv[k] + b * wwv[k] for k in range(3)])
    qn = _unit(_quat_mul(qt, exp_quat(w)))
    if sum(x * y for x, y in zip(qn, qt)) < 0:
        qn = [-c for c in qn]
    return [t[k] + p[k] for k in range(3)] + qn


def so3(q4, v3):
    return _unit(_quat_mul(_vec(q4), exp_quat(_vec(v3))))


def so2(cs, w):
    c0, s0 = _vec(cs)
    w = mpf(float(w))
    cw, sw = mp.cos(w), mp.sin(w)
    return _unit([c0 * cw - s0 * sw, s0 * cw + c0 * sw])


def se2(q4, v3):
    x, y, c0, s0 = _vec(q4)
    vx, vy, w = _vec(v3)
    if w == 0:
        tx, ty = vx, vy
    else:
        a, b = mp.sin(w) / w, 2 * mp.sin(w / 2) ** 2 / w
        tx, ty = a * vx - b * vy, b * vx + a * vy
    return [x + c0 * tx - s0 * ty, y + s0 * tx + c0 * ty] + so2(q4[2:4], v3[2])


def integrate(model, q, v):
    """q (+) v of one configuration [nq] and one velocity [nv], as doubles"""
    if getattr(model, "composite", None):
        return integrate(W._Chain(model), q, v)
    q, v = np.asarray(q, dtype=float), np.asarray(v, dtype=float)
    out = q.copy()
    mp.dps = DIGITS
    for i in range(1, model.njoints):
        jt, iq, iv = int(model.jtype[i]), int(model.idx_q[i]), int(model.idx_v[i])
        if jt == J_FREEFLYER:
            out[iq:iq + 7] = [float(c) for c in se3(q[iq:iq + 7], v[iv:iv + 6])]
        elif jt == J_SPHERICAL:
            out[iq:iq + 4] = [float(c) for c in so3(q[iq:iq + 4], v[iv:iv + 3])]
        elif jt == J_PLANAR:
            out[iq:iq + 4] = [float(c) for c in se2(q[iq:iq + 4], v[iv:iv + 3])]
        elif jt in (J_RUBX, J_RUBY, J_RUBZ, J_RUBU):
            out[iq:iq + 2] = [float(c) for c in so2(q[iq:iq + 2], v[iv])]
        else:
            n = int(W._NV.get(jt, 1))
            assert int(W._NQ.get(jt, 1)) == n, jt
            out[iq:iq + n] = q[iq:iq + n] + v[iv:iv + n]
    return out


def angular_dofs(model):
    """[(joint kind, first velocity index, count)] of the angular part of every joint that integrates on a group: the free-flyer's
    and the spherical joint's three, the planar joint's and the (cos, sin) joints' one"""
    if getattr(model, "composite", None):
        return angular_dofs(W._Chain(model))
    out = []
    for i in range(1, model.njoints):
        jt, iv = int(model.jtype[i]), int(model.idx_v[i])
        if jt == J_FREEFLYER:
            out.append((jt, iv + 3, 3))
        elif jt == J_SPHERICAL:
            out.append((jt, iv, 3))
        elif jt == J_PLANAR:
            out.append((jt, iv + 2, 1))
        elif jt in (J_RUBX, J_RUBY, J_RUBZ, J_RUBU):
            out.append((jt, iv, 1))
    return out


def unit_blocks(model):
    """[(first coordinate, count)] of every quaternion (count 4) and (cos, sin) pair (count 2) in q"""
    if getattr(model, "composite", None):
        return unit_blocks(W._Chain(model))
    out = []
    for i in range(1, model.njoints):
        jt, iq = int(model.jtype[i]), int(model.idx_q[i])
        if jt == J_FREEFLYER:
            out.append((iq + 3, 4))
        elif jt == J_SPHERICAL:
            out.append((iq, 4))
        elif jt == J_PLANAR:
            out.append((iq + 2, 2))
        elif jt in (J_RUBX, J_RUBY, J_RUBZ, J_RUBU):
            out.append((iq, 2))
    return out
