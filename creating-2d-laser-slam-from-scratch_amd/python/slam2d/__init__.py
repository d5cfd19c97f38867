"""slam2d: MI355X-native Hector scan-matching + occupancy-grid hot path (and the GMapping particle
grid path, PL-ICP, the Karto matcher, occupancy grid, pose-graph optimiser, loop-closure search and graph linking and the lesson5 lidar undistortion) of tonglf/Creating-2D-laser-slam-from-scratch, behind the C-ABI in include/slam2d/*.h.

Import is cheap; the HIP library is loaded on first use (slam2d._lib.lib()).
"""
from ._lib import LIB_PATH, Slam2dError, build, lib  # noqa: F401
from .karto_correct import PoseCorrection  # noqa: F401
from .karto_edit import GraphEdits  # noqa: F401
from .karto_grid import OccupancyGridBuilder  # noqa: F401
from .karto_link import LinkStage  # noqa: F401
from .karto_loop import LoopSearchFleet  # noqa: F401
from .karto_process import ProcessStage  # noqa: F401
from .spa import SpaFleet, SpaSolver  # noqa: F401
from .undistort import LidarUndistortion, UndistortFleet  # noqa: F401

__all__ = ["LIB_PATH", "Slam2dError", "build", "lib", "LidarUndistortion", "UndistortFleet", "OccupancyGridBuilder", "SpaFleet",
           "SpaSolver", "LoopSearchFleet", "LinkStage", "ProcessStage", "GraphEdits", "PoseCorrection"]
