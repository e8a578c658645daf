"""nyx_amd — MI355X-native batched propagation path behind the interface of nyx-space/nyx's
Propagator / MonteCarlo.  The numeric path is the HIP library
``nyx_amd/libnyx_hip.so`` (C-ABI in include/nyx_hip.h); importing this package does not load it,
any compute call does and fails loudly if it is missing."""
from . import _abi  # noqa: F401
from .propagator import *  # noqa: F401,F403
from ._abi import SCHED_CALIBRATED, SCHED_EXPLICIT, SCHED_MODEL, Tuning  # noqa: F401,E402
from .mc import AerSeries, DispersedState, EclipseSeries, FrameSeries, GroundTrackSeries, LinkSeries, MonteCarlo, MvnSpacecraft, PropResult, Results, RicSeries, Run, StateDispersion, ValueSeries, shard_bounds  # noqa: F401,E402
from .params import StateError, StateParameter, ric_difference, smooth_ric, state_value  # noqa: F401,E402
from .groundtrack import GroundTrackParameter, geodetic, ground_track_value, iau_dcm, to_body_fixed  # noqa: F401,E402
from .stations import AerParameter, GroundStation, aer_value, check_stations, station_consts  # noqa: F401,E402
from .frames import FrameParameter, body_state, cheby_state, frame_value, to_frame  # noqa: F401,E402
from .links import LinkParameter, check_link_bodies, link_value  # noqa: F401,E402
from .lambert import LambertGrid, LambertParameter, LambertSolution, LambertStatus, TransferKind, grid_definition, izzo  # noqa: F401,E402
from .targeter import BPlaneTarget, Objective, TargetStatus, Targeter, TargeterSolutions, Variable, Vary, target_definition  # noqa: F401,E402
from .stats import SeriesStats, Stat, series_stats  # noqa: F401,E402
from .eclipse import EclipseParameter, ShadowModel, check_shadow_model, eclipse_value, state_changes  # noqa: F401,E402
from .rng import Pcg64Mcg  # noqa: F401,E402
from .od import KalmanODProcess, Predicted, ProcessNoise3D, predict_until  # noqa: F401,E402
