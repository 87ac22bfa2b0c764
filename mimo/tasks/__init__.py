"""Mirrored here in part; sub-modules this tree lacks resolve from a reference checkout later on the path (mimo/__init__.py)."""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
