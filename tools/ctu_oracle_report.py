"""profiles/ctu_oracle_errors.txt from the output of tests/test_ctu_oracle.py (run with -s): one line per
case with the staged / tile / k_ctu_wave error and the contracted tile / k_ctu_wave error, on the emulator
and on the MI355X.

    python -m pytest tests/test_ctu_oracle.py -m "not gpu" -s -p no:xdist > emu.log
    python -m pytest tests/test_ctu_oracle.py -m gpu -s > gpu.log
    python tools/ctu_oracle_report.py emu.log gpu.log "<commit, box, date of the MI355X run>" [notes.txt] > profiles/ctu_oracle_errors.txt

notes.txt: lines appended as they are (measurements taken once, by hand, while the list was built).
"""
import re
import sys

CASE = re.compile(r"^\.?F?(\(\d+, \d+, \d+\)) (\(.*?\)): dt .*?; staged / tile / k_ctu_wave err (\S+) (\S+) (\S+), "
                  r"contracted tile / k_ctu_wave (\S+) (\S+)$")
BIG = re.compile(r"^\.?F?(\(\d+, \d+, \d+\)) (\(.*?\)) \((\w+)\) rows (\(.*?\)) columns (\(.*?\)): k_ctu_wave err (\S+), "
                 r"contracted (\S+)$")
COLD = re.compile(r"^\.?F?(limiter \d kernel_set \d fast_math \d): max \|U - oracle\| (\S+) \(bound (\S+)\)$")
STEPS = re.compile(r"^\.?F?(\(\d+, \d+, \d+\)) (\(.*?\)): three steps err (\S+), dt err (\S+)$")


def parse(path):
    one, big, steps, cold = {}, [], {}, {}
    for line in open(path):
        line = line.rstrip("\n")
        m = CASE.match(line)
        if m:
            one[m.group(1), m.group(2)] = m.groups()[2:]
        m = BIG.match(line)
        if m:
            big.append(m.groups())
        m = STEPS.match(line)
        if m:
            steps[m.group(1), m.group(2)] = m.groups()[2:]
        m = COLD.match(line)
        if m:
            cold[m.group(1)] = m.groups()[1:]
    return one, big, steps, cold


def main():
    emu, gpu, where = sys.argv[1], sys.argv[2], sys.argv[3]
    e1, _, es, ec = parse(emu)
    g1, gb, gs, gc = parse(gpu)
    print("# one step of the Cartesian CTU kernels against the C oracle (tests/test_ctu_oracle.py, cases: tests/ctu_cases.py).")
    print("# Per case (shape (nx, ny, march_rows); state, sides, limiter, flattening, grav, solver, small_dens):")
    print("#   exact: staged set / tile kernel / k_ctu_wave, bit-faithful build, per variable max |U - oracle| / max |oracle| over")
    print("#          the interior (bar: equal bits on the emulator, 1e-13 on the MI355X);")
    print("#   contracted: tile kernel / k_ctu_wave with fast_math = 1, element-wise |U - oracle| / (|oracle| + floor) with")
    print("#          conftest.comp_floors (bar 1e-10).  The emulator's contracted build divides exactly: its own algebra only.")
    print(f"# MI355X: {where}")
    worst = {"emulator": 0.0, "MI355X": 0.0}
    for key in e1:
        e, g = e1[key], g1.get(key)
        worst["emulator"] = max(worst["emulator"], float(e[3]), float(e[4]))
        if g:
            worst["MI355X"] = max(worst["MI355X"], float(g[3]), float(g[4]))
        print(f"{key[0]} {key[1]}: emulator exact {e[0]} {e[1]} {e[2]} contracted {e[3]} {e[4]}; "
              + (f"MI355X exact {g[0]} {g[1]} {g[2]} contracted {g[3]} {g[4]}" if g else "MI355X -"))
    print(f"# largest contracted error: emulator {worst['emulator']:.3e}, MI355X {worst['MI355X']:.3e}")
    print("# three steps of k_ctu_wave (bit-faithful) and comp_evolve against the oracle loop: state err, dt err")
    for key in es:
        g = gs.get(key)
        print(f"{key[0]} {key[1]}: emulator {es[key][0]} {es[key][1]}; " + (f"MI355X {g[0]} {g[1]}" if g else "MI355X -"))
    print("# the searched shapes of 256 compute units (MI355X only): k_ctu_wave equals the tile kernel bit for bit over the whole")
    print("# array; against the oracle on windows of rows x columns")
    for shape, case, path, rows, cols, err, ferr in gb:
        print(f"{shape} {case} {path} rows {rows} columns {cols}: exact {err} contracted {ferr}")
    print("# the regime the list keeps off: 14 x 30, `sedov`, HLLC, grav -0.3 (test_contracted_hllc_over_cold_gas_under_gravity):")
    print("# max |U - oracle| over the interior; the bound of the contracted builds comes from the oracle's face states")
    for key in ec:
        g = gc.get(key)
        print(f"{key}: emulator {ec[key][0]}, MI355X {g[0] if g else '-'} (bound {ec[key][1]})")
    if len(sys.argv) > 4:
        sys.stdout.write(open(sys.argv[4]).read())


if __name__ == "__main__":
    main()
