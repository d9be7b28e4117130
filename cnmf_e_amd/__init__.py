"""CNMF-E on AMD Instinct (gfx950).  The modules are imported by name (cnmf_e_amd.engine, .sources2d, .batch, ...); the names below are also reachable from the
package, resolved on first use so that `import cnmf_e_amd` (and cnmf_e_amd.build) works before the library is built."""

_EXPORTS = {"Sources2DBatch": "batch", "batch_frame_ranges": "batch"}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
