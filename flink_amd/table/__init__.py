"""Table/SQL window TVF aggregation (TUMBLE / HOP / CUMULATE / SESSION) on MI355X."""
from .session_window_agg import SessionWindowAggOperator  # noqa: F401
from .slice_assigners import SliceAssigners  # noqa: F401
from .window_agg import WindowAggOperator, is_gpu_eligible  # noqa: F401
