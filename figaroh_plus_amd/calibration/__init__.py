"""Geometric calibration: the kinematic regressor and updated forward kinematics (``calibration_tools``) and the D-optimal
selection of calibration postures (``optimal_design``)."""
from .optimal_design import (CandidatePool, Detmax, SOCP, detroot_whole, minNbChosen, rearrange_rb, select_configurations,
                             sub_info_matrix)

__all__ = ["CandidatePool", "Detmax", "SOCP", "detroot_whole", "minNbChosen", "rearrange_rb", "select_configurations",
           "sub_info_matrix"]
