"""``Robot`` -- mirror of ``src/figaroh/tools/robot.py:23-155`` without Pinocchio.

Same constructor arguments, same attributes the identification scripts read
(``.model .data .q0 .v0 .nq .nv``, ``model.nq/nv/njoints/names/inertias``,
``model.joints[j].idx_q/idx_v``; e.g. ``examples/tiago/identification.py:418-424``)
and the same ``get_standard_parameters`` ordering, which *is* the column order
of the regressor.  ``Robot.from_flat`` loads one of the flattened trees shipped
in ``figaroh_plus_amd/models`` so no URDF is needed at run time.
"""
import os

import numpy as np

from ..model import Model, build_model_from_urdf
from .robotcollisions import GeometryModel

_MODELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models")

PARAMS_NAME = ("Ixx", "Ixy", "Ixz", "Iyy", "Iyz", "Izz", "mx", "my", "mz", "m")
# Pinocchio dynamic-parameter slot [m mx my mz Ixx Ixy Iyy Ixz Iyz Izz] -> position inside a link block
# (robot.py:110-119); the regressor columns use the same permutation (regressor.py:72-82)
PIN_TO_FIG = (9, 6, 7, 8, 0, 1, 3, 2, 4, 5)


class Robot:
    def __init__(self, robot_urdf, package_dirs=None, isFext=False, freeflyer_ori=None, _model=None):
        self.params_name = PARAMS_NAME
        self.isFext = isFext
        self.robot_urdf = robot_urdf
        self.model = _model if _model is not None else build_model_from_urdf(robot_urdf, root_joint=isFext)
        if freeflyer_ori is not None and isFext:
            joint_id = self.model.getJointId("root_joint")
            self.model.jointPlacements[joint_id].rotation = np.array(freeflyer_ori, dtype=float)
            ub, lb = self.model.upperPositionLimit, self.model.lowerPositionLimit
            ub[:7] = 1
            lb[:7] = -1
        self.data = self.model.createData()
        self.q0 = self.model.neutral()
        self.v0 = np.zeros(self.model.nv)
        self.nq, self.nv = self.model.nq, self.model.nv
        self.geom_model = GeometryModel()  # collision objects and pairs (tools/robotcollisions.py), empty by default
        self._handle = None

    @classmethod
    def from_flat(cls, name_or_path, isFext=None):
        """Robot from a flattened tree: a file path or one of tx40 / ur10 / tiago / talos / human."""
        path = name_or_path
        if not os.path.exists(path):
            path = os.path.join(_MODELS, name_or_path + ".json")
        model = Model.from_flat(path)
        has_ff = model.njoints > 1 and model.joints[1].jtype == 3
        return cls(path, None, isFext=has_ff if isFext is None else isFext, _model=model)

    # ------------------------------------------------------------------ device handle (HIP library)
    def device_model(self):
        """figh_model_t for this tree, created on first use (fails loudly without the HIP library)."""
        if self._handle is None:
            from .. import _lib
            self._handle = _lib.ModelHandle(self.model.to_flat())
        return self._handle

    # ------------------------------------------------------------------ robot.py:76-155
    def get_standard_parameters(self, param):
        model = self.model
        phi, params = [], []
        for i in range(1, len(model.inertias)):
            P = model.inertias[i].toDynamicParameters()
            block = np.zeros(10)
            for src, dst in enumerate(PIN_TO_FIG):
                block[dst] = P[src]
            params += [name + str(i) for name in PARAMS_NAME]
            phi += list(block)
            params += ["Ia" + str(i), "fv" + str(i), "fs" + str(i), "off" + str(i)]
            for flag, keys, label in (("has_actuator_inertia", ("Ia",), "has_actuator_inertia_%d"),
                                      ("has_friction", ("fv", "fs"), "has_friction_%d"),
                                      ("has_joint_offset", ("off",), "has_joint_offset_%d")):
                if param[flag]:
                    try:
                        phi += [param[k][i - 1] for k in keys]
                    except Exception as e:  # the reference swallows short lists the same way (robot.py:130-134)
                        print("Warning: ", label % i, e)
                        phi += [0] * len(keys)
                else:
                    phi += [0] * len(keys)
        return dict(zip(params, phi))
