"""The problem setups are those of the advection solver (the reference links / copies the
same files under this solver's problems directory)."""
import importlib
import pkgutil
import sys

from ...advection import problems as _base

for _m in pkgutil.iter_modules(_base.__path__):
    sys.modules[f"{__name__}.{_m.name}"] = importlib.import_module(f"{_base.__name__}.{_m.name}")
