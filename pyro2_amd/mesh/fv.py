"""FV2d: cell-average data of the 4th-order finite-volume solvers, the class surface of
pyro/mesh/fv.py:1-39.  to_centers is analysis (host, NumPy); from_centers runs on the device
(pyrohip_state_from_centers)."""
from ..util import msg
from .patch import CellCenterData2d


class FV2d(CellCenterData2d):
    """a finite-volume grid whose data are cell averages; operations are 4th order and
    assume dx = dy"""

    def to_centers(self, name, is_positive=False):
        """variable `name` converted from averages to cell centres (fv.py:18-29): the raw
        average in the outermost ghost ring, a - dx^2 lap(a) / 24 inside it"""
        import numpy as np
        a = self.get_var(name)
        c = self.grid.scratch_array()
        ng = self.grid.ng
        c[:, :] = a[:, :]
        c.v(buf=ng - 1)[:, :] = a.v(buf=ng - 1) - self.grid.dx**2 * a.lap(buf=ng - 1) / 24.0
        if is_positive:
            c.v(buf=ng - 1)[:, :] = np.where(c.v(buf=ng - 1) >= 0.0, c.v(buf=ng - 1), a.v(buf=ng - 1))
        return c

    def from_centers(self, name):
        """treat the stored data as cell centres and convert them to averages (fv.py:31-39):
        ghost fill, then a + dx^2 lap(a) / 24 on the interior, on the device"""
        n = self.names.index(name)
        if self.slab is not None or self._has_host_bc(name):
            msg.fail("ERROR: from_centers runs on a single domain with device boundary rules")
        st = self.device_state()
        self._push_user_bc(st)
        st.from_centers(n, self.grid.dx, self.grid.dy)
        self.device_modified()
