"""Same-process-free A/B of two builds of the library on the headline call: python tools/ab_two_libs.py libA.so libB.so [reps]
(alternates subprocesses of tools/bench_headline_ab.py with LISFLOOD_AMD_LIBRARY set; "default" is the library in the tree,
and lib:VAR=VALUE[:VAR=VALUE...] sets environment switches for that side, e.g. default:LF_LEVEL_COUNTS=0).  A run that fails
or takes more than five minutes ends the comparison with its exit status: nothing more is started on the device."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
libs = sys.argv[1:3]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
for rep in range(reps):
    for side in libs:
        lib, *switches = side.split(":")
        env = dict(os.environ)
        if lib != "default":
            env["LISFLOOD_AMD_LIBRARY"] = os.path.abspath(lib)
        env.update(s.split("=", 1) for s in switches)
        try:
            run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_headline_ab.py"), "10000", "30"], env=env,
                                 capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            sys.exit("%s: no result after 300 s" % side)
        if run.returncode != 0:
            print(run.stderr[-2000:], file=sys.stderr)
            sys.exit(run.returncode if run.returncode > 0 else 1)
        print(side, "|", " | ".join(l.split(": ", 1)[1] for l in run.stdout.strip().splitlines() if ": " in l), flush=True)
