"""Handle object over the C ABI: one Engine per (device, stream) holds the packed weights,
spatial-model tables and workspace that the reference keeps as module globals + a
tf.Session (SURVEY.md 8b 'Implicit state').  torch is used only to own device buffers.
One module per subsystem, each a plain base class of Engine; _core (the handle and the shared helpers) is the only one the others import."""
from ..motion import SEQ_EXCLUDE      # noqa: F401  (the default of seq_tracks; engine.SEQ_EXCLUDE stays importable)
from ._core import Core, _hm_size      # noqa: F401
from .batches import Batches
from .images import Images
from .layers import Layers
from .sequence import Sequence
from .summaries import Summaries
from .tower import Tower


class Engine(Core, Layers, Tower, Sequence, Images, Batches, Summaries):
    """Owns a jcm_handle.  All tensor arguments are torch CUDA float32 NHWC, contiguous."""
