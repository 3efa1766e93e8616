"""Normalising flows of the hot path. The package is `flows` (plural): under the drop-in alias the reference's name
`models.flow` keeps its raising placeholder (compat.py)."""

from pytorch_generative_amd.models.flows import nice  # noqa: F401
