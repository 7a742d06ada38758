"""developer tool: what passive scalars cost the compressible tile kernel (GPU box).

    python tools/scalars_time.py [record.txt]        (profiles/scalars_time.txt)

The Sedov blast at 256^2, 1024^2 and 2048^2 (SIZES) with 0, 1 and 2 passive scalars behind the
four hydro variables (fuel = rho (0.5 + 0.4 sin 2 pi x cos 2 pi y), ash = rho - fuel), stepped by
DeviceState.comp_step on kernel_set 1 -- the tile kernel k_ctu_fused, the ghost fill folded into
the launch -- in both arithmetic builds, all in one session.  The warm-up convention of
tools/burgers_time.py (leg 2): K_WARM calls untimed, then REPS repetitions of K_CALLS calls; the
kernel's own time from the library's event timing (Context.prof_report) and the wall clock per
call with a synchronisation at both ends.

Yardsticks: the NA = 0 tile kernel of the same session, and the HBM floor of 16 (4 + NA) bytes per
cell at 8 TB/s.  A row whose NA = 2 time exceeds 2 (4 + NA) / 4 = 3 times the NA = 0 time is
flagged: that is the threshold for writing the kernel's registers and LDS down in DESIGN.md as the
next thing to look at, not a gate."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                    # noqa: E402

from pyro2_amd import device                                          # noqa: E402
from pyro2_amd.compressible.problems.sedov import sedov_state        # noqa: E402

SIZES = [int(x) for x in os.environ.get("SIZES", "256,1024,2048").split(",")]
REPS = int(os.environ.get("REPS", "3"))
K_WARM = int(os.environ.get("K_WARM", "5"))
K_CALLS = int(os.environ.get("K_CALLS", "20"))
NG = 4


def state(ctx, nx, na):
    U4 = sedov_state(nx, nx, NG, 0.0, 1.0, 0.0, 1.0, 1.4, 0.1, 4)
    U = np.empty(U4.shape[:2] + (4 + na,))
    U[..., :4] = U4
    x = (np.arange(nx + 2 * NG) - NG + 0.5) / nx
    X = 0.5 + 0.4 * np.sin(2 * np.pi * x)[:, None] * np.cos(2 * np.pi * x)[None, :]
    if na >= 1:
        U[..., 4] = U4[..., 0] * X
    if na == 2:
        U[..., 5] = U4[..., 0] - U[..., 4]
    rows = [["outflow"] * 4] * (4 + na)
    st = device.DeviceState(ctx, nx, nx, NG, rows)
    st.upload(U)
    st.fill_bc()
    return st


def measure(ctx, nx, na, fm):
    st = state(ctx, nx, na)
    P = device.make_comp_params(1.0 / nx, 1.0 / nx, fast_math=fm, kernel_set=1, fuse_fill=1)
    dt = 0.01 * st.comp_dt(P, 0.8)
    for _ in range(K_WARM):
        st.comp_step(P, dt)
    ctx.sync()
    kms, wms = [], []
    for _ in range(REPS):
        ctx.prof_report()
        ctx.prof_enable(True)
        for _ in range(K_CALLS):
            st.comp_step(P, dt)
        ctx.sync()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        assert set(rep) == {"k_ctu_fused"} and rep["k_ctu_fused"][0] == K_CALLS, rep
        kms.append(rep["k_ctu_fused"][1] / K_CALLS)
        t0 = time.perf_counter()
        for _ in range(K_CALLS):
            st.comp_step(P, dt)
        ctx.sync()
        wms.append(1e3 * (time.perf_counter() - t0) / K_CALLS)
    assert np.all(np.isfinite(st.download()[NG:-NG, NG:-NG]))
    return kms, wms


def fmt(ms):
    return f"median {np.median(ms):8.4f} ms   spread {max(ms) - min(ms):7.4f}   runs " + " ".join(f"{m:.4f}" for m in ms)


def main():
    rec = [a for a in sys.argv[1:] if not a.startswith("--")]
    ctx = device.Context.default()

    def say(line):
        print(line, flush=True)
        if rec:
            with open(rec[0], "a") as f:
                f.write(line + "\n")
    say(f"scalars_time: Sedov, kernel_set 1 (k_ctu_fused), fuse_fill; {K_WARM} warm-up calls + {REPS} repetitions of "
        f"{K_CALLS} calls; ms per call   {time.strftime('%Y-%m-%d')}   {ctx.info()['name']}")
    for fm in (1, 0):
        say(f"fast_math {fm} ({'contracted' if fm else 'bit-faithful'} build)")
        for nx in SIZES:
            med = {}
            for na in (0, 1, 2):
                kms, wms = measure(ctx, nx, na, fm)
                med[na] = float(np.median(kms))
                floor = 16.0 * (4 + na) * nx * nx / 8.0e12 * 1e3
                say(f"{nx:5d}^2 NA {na}: kernel " + fmt(kms))
                say(f"{'':14}  wall   " + fmt(wms) + f"   HBM floor {floor:.4f} ms   x NA 0: {med[na] / med[0]:.2f}")
            if med[2] > 3.0 * med[0]:
                say(f"{nx:5d}^2 NA 2 COSTS MORE THAN (4 + NA) / 4 x 2 = 3 TIMES NA 0: record in DESIGN.md")
    say("")


if __name__ == "__main__":
    main()
