"""DataStream window operators on MI355X: event-time windows (tumbling / sliding + built-in
sum/min/max), count windows (countWindow, also emitting whole records) and event-time session windows (static gap, dynamic gap, allowed lateness, dynamic gap with allowed lateness)."""
from .windowing import EventTimeTrigger, SlidingEventTimeWindows, TumblingEventTimeWindows  # noqa: F401
from .windowing import CountEvictor, CountTrigger, GlobalWindows, PurgingTrigger  # noqa: F401
from .windowing import DynamicEventTimeSessionWindows, EventTimeSessionWindows  # noqa: F401
from .window_operator import WindowOperator, is_gpu_eligible  # noqa: F401
from .count_window_operator import CountWindowOperator  # noqa: F401
from .count_window_operator import is_gpu_eligible as is_count_window_gpu_eligible  # noqa: F401
from .record_count_window_operator import RecordCountWindowOperator  # noqa: F401
from .record_count_window_operator import is_gpu_eligible as is_record_count_window_gpu_eligible  # noqa: F401
from .session_window_operator import SessionWindowOperator  # noqa: F401
from .session_window_operator import is_gpu_eligible as is_session_window_gpu_eligible  # noqa: F401
from .dynamic_session_window_operator import DynamicSessionWindowOperator  # noqa: F401
from .dynamic_session_window_operator import is_gpu_eligible as is_dynamic_session_window_gpu_eligible  # noqa: F401
from .late_session_window_operator import LateSessionWindowOperator  # noqa: F401
from .late_session_window_operator import is_gpu_eligible as is_late_session_window_gpu_eligible  # noqa: F401
from .late_dynamic_session_window_operator import LateDynamicSessionWindowOperator  # noqa: F401
from .late_dynamic_session_window_operator import is_gpu_eligible as is_late_dynamic_session_window_gpu_eligible  # noqa: F401
from .session_exchange import SessionExchangeStep  # noqa: F401
from .count_exchange import CountExchangeStep  # noqa: F401
from .record_count_exchange import RecordCountExchangeStep  # noqa: F401
