"""Atmosphere: the altitude-dependent density model of the drag (include/mpcx.h, mpcx_set_atmosphere / MPCX_FLAG_ATMO).

One closed form with four coefficients {c0, c1, c2, h_floor} in physical units,

    alt = |r R0| - R_EARTH            metres, the altitude of Simulator.get_atmo_density (reference simulator.py:109)
    h   = max(alt, h_floor)
    rho(h) = exp(c0 + c1 ln h + c2 h)                       kg/m^3
    d rho / d h = rho (c1 / h + c2)  above the floor, 0 on it

which holds the Harris-Priester power fit the reference keeps commented out as "too slow" (simulator.py:110) and the
exponential atmosphere.  The device evaluates it in every right-hand side of the rollouts and of the linearisation; the numpy
evaluation here is the same formula, for callers that want the numbers and for the reference's own Discretizer
(reference_funcs)."""
import math

import numpy as np

from .constants import R_EARTH


class Atmosphere:
    def __init__(self, c0, c1, c2, h_floor):
        self.c0, self.c1, self.c2, self.h_floor = float(c0), float(c1), float(c2), float(h_floor)
        if not all(math.isfinite(v) for v in self.coefficients()):
            raise ValueError("Atmosphere: coefficients must be finite")
        if not self.h_floor > 0.0:
            raise ValueError("Atmosphere: h_floor must be > 0 (it keeps ln h defined wherever a trial stage of the integrator lands)")

    @classmethod
    def power_law(cls, a=8e26, b=6.828, h_floor=1e5):
        """rho = a h^-b; the defaults are the reference's fit of the Harris-Priester table (simulator.py:110)"""
        return cls(math.log(a), -float(b), 0.0, h_floor)

    @classmethod
    def exponential(cls, rho_ref, h_ref, H, h_floor=1e5):
        """rho = rho_ref exp(-(h - h_ref) / H), scale height H in metres"""
        return cls(math.log(rho_ref) + h_ref / H, 0.0, -1.0 / H, h_floor)

    def coefficients(self):
        """(c0, c1, c2, h_floor): atmo[MPCX_NATMO] of mpcx_set_atmosphere"""
        return (self.c0, self.c1, self.c2, self.h_floor)

    def _h(self, alt):
        alt = np.asarray(alt)
        above = alt.real > self.h_floor
        return np.where(above, alt, self.h_floor), above

    def density(self, alt):
        """rho at altitude(s) alt in metres, kg/m^3 (complex alt: for a complex-step derivative)"""
        h, _ = self._h(alt)
        return np.exp(self.c0 + self.c1 * np.log(h) + self.c2 * h)

    def ddensity(self, alt):
        """d rho / d h at altitude(s) alt: 0 on the floor"""
        h, above = self._h(alt)
        return np.where(above, self.density(alt) * (self.c1 / h + self.c2), 0.0)

    def reference_funcs(self, const):
        """(rho_func, drho_func) in the convention of the reference's Discretizer (linearize_discretize.py:164-166): the
        normalised position in; rho / const.RHO and its derivative with respect to the normalised radius out."""
        r0, rho_n = float(const.R0), float(const.RHO)

        def altitude(r):
            return np.linalg.norm(np.asarray(r) * r0) - R_EARTH

        def rho_func(r):
            return self.density(altitude(r)) / rho_n

        def drho_func(r):
            return self.ddensity(altitude(r)) * r0 / rho_n
        return rho_func, drho_func

    def __repr__(self):
        return f"Atmosphere(c0={self.c0!r}, c1={self.c1!r}, c2={self.c2!r}, h_floor={self.h_floor!r})"
