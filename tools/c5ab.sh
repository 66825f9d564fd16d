cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
# logs go to $ZP_OUT (default bench_out/, ignored by git)
O=${ZP_OUT:-bench_out}
mkdir -p $O
for i in 1 2; do
  timeout -k 10 300 python bench.py --full > $O/c5ab_default_$i.log 2>&1 || exit $?
  timeout -k 10 300 python bench.py --full --no-pcie > $O/c5ab_nopcie_$i.log 2>&1 || exit $?
  timeout -k 10 300 python bench.py --full --no-cpu > $O/c5ab_nocpu_$i.log 2>&1 || exit $?
done
