"""How the golden makers load the reference's own Python files: by path, under stand-in modules of this project's writing."""
import importlib.util
import os
import sys


def load_under_stand_ins(root, files, stand_ins):
    """Execute `files` ((module name, path below root), in order) with `stand_ins` ({module name: module}) in sys.modules, so that
    their imports find the stand-ins and each other; sys.modules is as it was afterwards.  Returns {module name: module}."""
    saved = {k: sys.modules.get(k) for k in list(stand_ins) + [name for name, _ in files]}
    sys.modules.update(stand_ins)
    mods = {}
    try:
        for name, path in files:
            spec = importlib.util.spec_from_file_location(name, os.path.join(root, path))
            mods[name] = importlib.util.module_from_spec(spec)
            sys.modules[name] = mods[name]
            spec.loader.exec_module(mods[name])
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods
