"""What the three ensemble classes share: the lifecycle of a handle that owns its jobs, and kernel_times' dictionary."""
from __future__ import annotations

from ._lib import lib


class _EnsembleBase:
    """``self.h`` (the C handle), ``self.jobs`` (views the handle owns) and ``_DESTROY`` (the C destructor's name)"""

    _DESTROY = ""

    def close(self):
        if getattr(self, "h", None):
            for j in self.jobs:
                j.close()
            getattr(lib(), self._DESTROY)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return len(self.jobs)

    @staticmethod
    def _times(out, keys, start=0):
        """{key: out[start + i]} with the launch counts (``n_*``) as ints"""
        return {k: (int(out[start + i]) if k.startswith("n_") else out[start + i]) for i, k in enumerate(keys)}
