"""Own URDF parse + forward kinematics of the AlienGo+Z1 model: the ONE geometry the independent pins are built on (tests/golden/make_model_fixture.py ->
model_independent.npz; tests/lq_reference.py).  Shares nothing with the product's loader, the oracle or the kernels: xml.etree on
qm_door_amd/data/aliengo_z1.urdf, all 28 links kept as separate bodies (no merging of fixed children), Rodrigues rotations.  Everything here is
holomorphic in q, so a complex step through fk is an exact derivative; fk also takes a batch of configurations (q [..., 24])."""
import os
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
URDF = os.path.join(HERE, "..", "qm_door_amd", "data", "aliengo_z1.urdf")
JOINT_ORDER = [f"{leg}_{j}" for leg in ("LF", "LH", "RF", "RH") for j in ("HAA", "HFE", "KFE")] + [f"z1_joint_{i}" for i in range(1, 7)]
FEET = ("LF", "RF", "LH", "RH")     # contact order of the MPC
EE_LINK = "z1_end_effector"


def parse():
    root = ET.parse(URDF).getroot()
    links = {}
    for l in root.findall("link"):
        inert = l.find("inertial")
        if inert is None:
            links[l.get("name")] = dict(m=0.0, c=np.zeros(3), I=np.zeros((3, 3)))
            continue
        i = inert.find("inertia")
        I = np.array([[float(i.get("ixx")), float(i.get("ixy")), float(i.get("ixz"))], [float(i.get("ixy")), float(i.get("iyy")), float(i.get("iyz"))],
                      [float(i.get("ixz")), float(i.get("iyz")), float(i.get("izz"))]])
        assert inert.find("origin").get("rpy").split() == ["0", "0", "0"]
        links[l.get("name")] = dict(m=float(inert.find("mass").get("value")), c=np.array(inert.find("origin").get("xyz").split(), float), I=I)
    joints = []
    for j in root.findall("joint"):
        o = j.find("origin")
        assert [float(t) for t in o.get("rpy").split()] == [0.0, 0.0, 0.0]
        ax = j.find("axis")
        lim = j.find("limit")
        joints.append(dict(name=j.get("name"), type=j.get("type"), parent=j.find("parent").get("link"), child=j.find("child").get("link"),
                           xyz=np.array(o.get("xyz").split(), float), axis=None if ax is None else np.array(ax.get("xyz").split(), float),
                           lower=None if lim is None or lim.get("lower") is None else float(lim.get("lower")),
                           upper=None if lim is None or lim.get("upper") is None else float(lim.get("upper"))))
    return links, joints


LINKS, JOINTS = parse()
CHILDREN = {}
for jt in JOINTS:
    CHILDREN.setdefault(jt["parent"], []).append(jt)


def rot(axis, a):
    """Rodrigues rotation about a unit axis; works for complex angles (complex step) and for a batch of angles (a [...] -> [..., 3, 3])."""
    x, y, z = axis
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], dtype=complex)
    a = np.asarray(a)[..., None, None]
    return np.eye(3, dtype=complex) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def fk(q):
    """world pose (R, p) of every link for generalised coordinates q (possibly complex, possibly a batch [..., 24])."""
    q = np.asarray(q, dtype=complex)
    R0 = rot((0, 0, 1), q[..., 3]) @ rot((0, 1, 0), q[..., 4]) @ rot((1, 0, 0), q[..., 5])
    pose = {"base": (R0, q[..., 0:3].copy())}
    stack = ["base"]
    while stack:
        parent = stack.pop()
        Rp, pp = pose[parent]
        for jt in CHILDREN.get(parent, []):
            ang = q[..., 6 + JOINT_ORDER.index(jt["name"])] if jt["name"] in JOINT_ORDER else 0.0
            Rc = Rp @ rot(jt["axis"], ang) if jt["type"] == "revolute" else Rp
            pose[jt["child"]] = (Rc, pp + Rp @ jt["xyz"])
            stack.append(jt["child"])
    return pose
