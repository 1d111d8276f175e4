"""Ranking models with the reference's plugin contract (ultra.ranking_model.*), HIP-backed."""
from .dnn import DNN, Linear, init_flat_params  # noqa: F401
from . import SetRank  # noqa: F401,E402  module, as in the reference: the class is ultra.ranking_model.SetRank.SetRank
from .DLCM import DLCM  # noqa: F401,E402  the CLASS, as the reference's settings spell it: ultra.ranking_model.DLCM
from .GSF import GSF  # noqa: F401,E402  the CLASS, likewise: ultra.ranking_model.GSF
