#!/bin/bash
# Build the library of an earlier commit (default: HEAD's parent) as an A/B variant and record the cases of
# tests/split_bitwise_cases.py on it into tests/golden/split_bitwise_parent.golden (+ .txt: the csrc hash it came from).
#   scripts/make_split_golden.sh build [<commit>]    export <commit>'s csrc + include and `make variant VARNAME=parent` there
#                                                     -> scripts/bin/libmcpc_parent.so (needs git and hipcc, no GPU)
#   scripts/make_split_golden.sh record              run the cases on scripts/bin/libmcpc_parent.so (needs the GPU, no git)
# Two steps because the library is built where the sources' history is and run where the GPU is.
set -e
cd "$(dirname "$0")/.."
case "$1" in
build)
    commit=${2:-HEAD~1}
    tmp=$(mktemp -d)
    git archive "$commit" montecarlopredictivecoding_amd/csrc include | tar -x -C "$tmp"
    mkdir -p "$tmp/scripts/bin" scripts/bin
    make -s -C "$tmp/montecarlopredictivecoding_amd/csrc" variant VARNAME=parent COMMIT="$(git rev-parse --short "$commit")"
    cp "$tmp/scripts/bin/libmcpc_parent.so" scripts/bin/libmcpc_parent.so
    rm -rf "$tmp"
    ls -la scripts/bin/libmcpc_parent.so
    ;;
record)
    MCPC_LIB=$PWD/scripts/bin/libmcpc_parent.so timeout -k 10 300 python3 scripts/make_split_golden.py record tests/golden/split_bitwise_parent.golden
    ;;
*)
    sed -n '2,8p' "$0"; exit 2
    ;;
esac
