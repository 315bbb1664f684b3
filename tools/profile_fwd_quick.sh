set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=gpurun_out/fz
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/stats -o t --output-format csv -- python3 bench.py --full --no-knn --no-cpu --no-graph-replay > $O/out.txt 2> $O/err.txt
