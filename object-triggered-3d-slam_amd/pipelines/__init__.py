"""open3d.pipelines counterpart: integration (the reconstruction scripts) and registration (the evaluation
scripts' ICP alignment)."""
from . import integration, registration  # noqa: F401
