"""How long a molecule takes to load (Kernel.load_molecule: PDBReader::loadAtomsFromFile) and where the time goes, on
synthetic PDB files of 486 ... 200 000 atoms at protein-like density (uniform, 2.74^3 of room an atom: about one other
atom within the stick reach of 1.7, about eight within a backbone's 3.4).

    python tools/molecule_load_time.py [--sizes 486,5000,20000,50000,200000] [--types 5,3] [--engine hip]
                                       [--output profiles/r27/molecule_sticks.txt]

Per file and geometry type (5 keys the reader's map by position in the file, so no atom is lost to the four-digit serial
field; 3 is the default of scenes.pdb_molecule and keys half the residues by serial number) it prints
    load       wall time of load_molecule
    atoms-only wall time of load_molecule of the same file with geometry type 0: the same parse, a sphere an atom, no sticks
    sticks     load - atoms-only: the search for the sticks and their cylinders added - measurable on any commit
    parse / search / emit   the reader's own clock for its three steps (Kernel.molecule_load_times), where the library has it
    compact    wall time of compact_boxes(True) behind the load
It uses only load_molecule and compact_boxes unless the library offers more, so the same file runs on an older commit for
a comparison: run both alternately in one session on one device."""
import argparse
import importlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_pdb(path, n, seed=1):
    rng = np.random.default_rng(seed)
    side = 2.74 * n ** (1.0 / 3.0)
    positions = rng.uniform(-side / 2, side / 2, (n, 3))
    with open(path, "w") as out:
        for i, (x, y, z) in enumerate(positions):
            line = [" "] * 80

            def put(at, text):
                line[at:at + len(text)] = text

            put(0, "ATOM")
            put(7, "%4d" % ((i + 1) % 10000))
            put(13, "CNO"[i % 3] + "A" * (i % 2))
            put(17, "ALA")
            put(21, "AB"[(i // 700) % 2])
            put(23, "%3d" % ((i // 7) % 1000))
            put(30, "%8.3f" % x)
            put(38, "%8.3f" % y)
            put(46, "%8.3f" % z)
            put(76, " " + "CNO"[i % 3])
            out.write("".join(line) + "\n")


def load(solr, engine, path, geometry_type, compact):
    k = solr.Kernel(engine=engine, deterministic_seed=1)
    k.initialize(width=64, height=48)
    for _ in range(1100):
        k.add_material(0.5, 0.5, 0.5)
    t0 = time.perf_counter()
    k.load_molecule(path, geometry_type=geometry_type, atom_size=100.0, stick_size=10.0, material_type=0, scale=200.0)
    t1 = time.perf_counter()
    steps = k.molecule_load_times() if hasattr(k, "molecule_load_times") else None
    searches = k.stick_searches() if hasattr(k, "stick_searches") else None
    t2 = t3 = 0.0
    nb = 0
    if compact:
        solr.scenes.add_light(k, position=(-5000.0, 5000.0, -15000.0), radius=1.0)
        t2 = time.perf_counter()
        k.compact_boxes(True)
        t3 = time.perf_counter()
        nb = len(k.flat_scene().primitives)
    k.finalize()
    return t1 - t0, steps, t3 - t2, nb, searches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="486,5000,20000,50000,200000")
    ap.add_argument("--types", default="5,3")
    ap.add_argument("--engine", default="hip")
    ap.add_argument("--label", default="")
    ap.add_argument("--device-from", type=int, default=None,
                    help="Kernel.set_stick_device_from: 0 searches on the device always, a large number never")
    ap.add_argument("--output", default="")
    args = ap.parse_args()
    solr = importlib.import_module("sol-r_amd")
    if args.engine == "hip" and solr.hip_lib().solr_hip_device_count() < 1:
        sys.exit("molecule_load_time.py: no GPU; nothing measured (try --engine host-only)")
    if args.device_from is not None:
        solr.Kernel(engine=args.engine).set_stick_device_from(args.device_from)
    lines = ["tools/molecule_load_time.py %s: engine %s%s; host clock, seconds"
             % (args.label, args.engine, "" if args.device_from is None else ", device from %d atoms" % args.device_from)]
    print(lines[0], flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for n in [int(s) for s in args.sizes.split(",")]:
            path = os.path.join(tmp, "synthetic_%d.pdb" % n)
            write_pdb(path, n)
            if n == int(args.sizes.split(",")[0]):
                load(solr, args.engine, path, 5, False)             # the first call of a process pays for loading the kernels
            plain = min(load(solr, args.engine, path, 0, False)[0] for _ in range(2))
            for geometry_type in [int(s) for s in args.types.split(",")]:
                total, steps, compact, nb, searches = load(solr, args.engine, path, geometry_type, True)
                line = "atoms %7d type %d: load %9.4f  atoms-only %8.4f  sticks %9.4f" % (n, geometry_type, total, plain,
                                                                                         total - plain)
                if steps:
                    line += "  | parse %8.4f search %9.4f emit %8.4f" % steps
                line += "  | compact %8.4f  primitives %8d" % (compact, nb)
                if searches:
                    line += "  searches (device, host) %s" % (searches,)
                lines.append(line)
                print(line, flush=True)
    if args.output:
        with open(args.output, "a") as out:
            out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
