"""usage (GPU box): python scripts/ab_headline.py <rounds> <out.jsonl> <libA> <libB> ...
Alternates engine builds (NFA_ENGINE_LIB) over <rounds> rounds of the plain bench command at (--steps, --warmup) = (200, 20)
and (20, 5); appends one line per run to <out.jsonl> and prints median / min / max of `value` per build: box and clock
drift hit all builds alike.  (scripts/gpu_ab.sh does the same for the pipelined rate of --full.)"""
import json, os, statistics as st, subprocess, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
rounds, out, libs = int(sys.argv[1]), sys.argv[2], sys.argv[3:]
rows = []
with open(out, 'a') as f:
    for r in range(rounds):
        for lib in libs:
            for K, W in ((200, 20), (20, 5)):
                env = dict(os.environ, NFA_ENGINE_LIB=os.path.abspath(lib))
                p = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--gpus', '1', '--steps', str(K), '--warmup', str(W)],
                                   env=env, capture_output=True, text=True, timeout=180)
                if p.returncode != 0:
                    sys.exit(f'bench failed ({lib}, K={K}): {p.returncode}\n{p.stderr[-2000:]}')
                row = {'round': r, 'build': Path(lib).stem, 'K': K, 'W': W, 'value': json.loads(p.stdout.strip().splitlines()[-1])['value']}
                rows.append(row)
                f.write(json.dumps(row) + '\n')
                f.flush()
for K in (200, 20):
    for lib in libs:
        v = [x['value'] / 1e6 for x in rows if x['build'] == Path(lib).stem and x['K'] == K]
        print(f'K={K:3d} {Path(lib).stem:24s} n={len(v)} median {st.median(v):7.2f} M  min {min(v):7.2f}  max {max(v):7.2f}')
