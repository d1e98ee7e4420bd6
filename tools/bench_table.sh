#!/bin/bash
# The workload table of DESIGN.md 4.5: bench.py over the other BASELINE shapes (run through gpurun from the repo root).
J='import json,sys; d=json.loads(sys.stdin.readline()); r=d["roofline"]; print("| %s | %.0f | %.2f ms | %.2f |" % (sys.argv[1], d["value"], d["ms_per_step"], r["frac"]))'
# each shape twice, the better line kept: the first process that touches a new slab size on a fresh box runs up to 15 % slow
J2='import json,sys; a=[json.loads(l) for l in sys.stdin if l.startswith("{")]; d=max(a,key=lambda x:x["value"]); r=d["roofline"]; print("| %s | %.0f | %.2f ms | %.2f |" % (sys.argv[1], d["value"], d["ms_per_step"], r["frac"]))'
run() { name=$1; shift; for i in 1 2; do python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --no-fed4k --no-single --no-match --no-self-check "$@" 2>/dev/null | grep '^{'; done | python3 -c "$J2" "$name"; }
run "32 x 1920x1080 per step (bench default)"
run "32 x 1920x1080, second-derivative / Lstep planes not kept (--lean)" --lean
run "1 x 1920x1080 per step" --frames 1
run "8 x 3840x2160 per step" --width 3840 --height 2160 --frames 8
run "1 x 3840x2160 per step" --width 3840 --height 2160 --frames 1
run "8 x 3840x2160, 5 octaves x 5 sublevels" --width 3840 --height 2160 --frames 8 --sublevels 5 --octaves 5
run "16 x 2016x1512 (size of the reference's test-data/1.jpg)" --width 2016 --height 1512 --frames 16
