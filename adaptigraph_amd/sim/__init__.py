"""Batched particle simulators, a rope on a table, a pile of discs pushed by a board, a cloth dragged by a gripper and a rigid box with a hidden centre
of mass: the data side of the workflow.  One module per model -- rope.py, pile.py, cloth.py, box.py -- each
with its parameters and scene, its host statement (`*_push_host`, float32 numpy: the SPECIFICATION, in the module's text), the same model in
scalars (`*_push_scalar`), its device call and `*_push` (one HIP launch, the same bits) and its scene and push samplers; _common.py holds what they
share.  Every name of the five that does not begin with an underscore is a name of this package (none of them defines __all__)."""
from ._common import *  # noqa: F401,F403
from .rope import *  # noqa: F401,F403
from .pile import *  # noqa: F401,F403
from .cloth import *  # noqa: F401,F403
from .box import *  # noqa: F401,F403
