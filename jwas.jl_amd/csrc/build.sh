#!/bin/bash
# Builds libjwas_hip.so for gfx950 in-tree (the .so travels with the gpurun snapshot).
# -ffp-contract=off: the arithmetic contract shared with the oracle (no implicit FMA contraction).
# Translation units, compiled in parallel: one per sampler family (step_*.hip, step_launch.hpp), one per device session
# (session_NAME.hip: its entry points on ctx.hpp's shared plumbing, its kernels in NAME.hpp), output.hip (the output side of both
# precisions and the GWAS session, kernels in output.hpp) and jwas_hip.hip (the context, storage, blocks, the sweep).  An object is
# rebuilt only when it is older than a source it includes -- a change in one session's kernels recompiles that session alone
# (INCREMENTAL=0 forces everything).
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OBJ=${JWAS_OBJ_DIR:-_obj}
OUT=${JWAS_OUT:-libjwas_hip.so}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $JWAS_EXTRA_FLAGS"
UNITS="jwas_hip output session_liability session_locpar session_mtmiss session_annot session_sem session_rrm session_mega session_mtjoint session_ssbr session_gblup session_plink step_st step_mtc1 step_mtb1 step_mt2 step_mega"
mkdir -p "$OBJ"
echo "$FLAGS $*" > "$OBJ/.flags.new"
if [ "${INCREMENTAL:-1}" = 0 ] || ! cmp -s "$OBJ/.flags.new" "$OBJ/.flags"; then rm -f "$OBJ"/*.o; fi
mv "$OBJ/.flags.new" "$OBJ/.flags"
needs() {      # does unit $1 have to be compiled?
    local o="$OBJ/$1.o"
    [ -f "$o" ] || return 0
    local deps="$1.hip ../../include/jwas_hip.h"
    local ctx="ctx.hpp device_util.hpp rng.hpp"      # ctx.hpp and what it includes
    local sweep="kernels.hpp rng.hpp sweep.hpp update_role.hpp sampler_common.hpp sampler_st.hpp sampler_mt.hpp step_launch.hpp"
    case $1 in
        jwas_hip)  deps="$deps $ctx $sweep f64_path.hpp output.hpp sweep_plan.hpp" ;;
        output)    deps="$deps $ctx kernels.hpp rng.hpp output.hpp" ;;
        session_rrm) deps="$deps $ctx marker_state.hpp rrm.hpp" ;;
        session_mega) deps="$deps $ctx marker_state.hpp block_session.hpp mega.hpp" ;;
        session_mtjoint) deps="$deps $ctx marker_state.hpp block_session.hpp mtjoint.hpp mega.hpp" ;;      # (the block form it runs on is mega.hpp's)
        session_*) deps="$deps $ctx ${1#session_}.hpp" ;;
        *)         deps="$deps $sweep step_launch_impl.hpp" ;;
    esac
    for d in $deps; do [ "$d" -nt "$o" ] && return 0; done
    return 1
}
pids=""
for u in $UNITS; do
    if needs $u; then
        "$HIPCC" $FLAGS "$@" -c $u.hip -o "$OBJ/$u.o" &
        pids="$pids $!"
    fi
done
for p in $pids; do wait $p; done
objs=""
for u in $UNITS; do objs="$objs $OBJ/$u.o"; done
"$HIPCC" --offload-arch=gfx950 -fPIC -shared $objs -o "$OUT"
