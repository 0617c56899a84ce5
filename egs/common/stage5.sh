#!/usr/bin/env bash
# Stage 5 (objective evaluation) of the jatts recipes on the MI355X path.  Sourced by egs/*/tts*/run.sh with the reference's variables
# set: expdir, checkpoint, test_set, eval_metrics (reference egs/jsut/tts1/run.sh:262-278) and, on JVS, spkemb_checkpoint.  Writes
# ${expdir}/results/<checkpoint>/<set>/evaluation.log and closes with the reference's grep for the "Mean" line.  eval_metrics defaults to
# what this package computes: mcd, plus spkemb where spkemb_checkpoint is set; asr and sheet are refused by name
# (jatts_amd.bin.evaluate).  The numbers are of jatts_amd's own definition (jatts_amd/evaluate.py): comparable between systems evaluated
# here, not with the numbers the reference's stage 5 prints.  eval_batch_size (optional recipe variable): pairs per ragged batch.
# shellcheck disable=SC2154
stage5_evaluate() {
    # shellcheck disable=SC2012
    [ -z "${checkpoint}" ] && checkpoint="$(ls -dt "${expdir}"/*.pkl | head -1 || true)"
    [ -n "${checkpoint}" ] || { log "no checkpoint under ${expdir}"; exit 1; }
    outdir="${expdir}/results/$(basename "${checkpoint}" .pkl)"
    local metrics="${eval_metrics:-}"
    if [ -z "${metrics}" ]; then
        metrics="mcd"
        [ -n "${spkemb_checkpoint:-}" ] && metrics="mcd spkemb"
    fi
    local name="${test_set}"
    local wavdir="${outdir}/${name}/wav"
    [ -d "${wavdir}" ] || { log "${wavdir} does not exist: run stage 4 first"; exit 1; }
    log "Evaluation start. See the progress via ${outdir}/${name}/evaluation.log."
    # shellcheck disable=SC2086
    "${python}" -m jatts_amd.bin.evaluate \
        --csv "data/${test_set}.csv" \
        --wavdir "${wavdir}" \
        --f0_path "conf/f0.yaml" \
        --batch-size "${eval_batch_size:-16}" \
        ${spkemb_checkpoint:+--spkemb_checkpoint "${spkemb_checkpoint}"} \
        --json "${outdir}/${name}/evaluation.json" \
        --metrics ${metrics} > "${outdir}/${name}/evaluation.log" 2>&1 || { tail -20 "${outdir}/${name}/evaluation.log"; exit 1; }
    grep "INFO: Mean" "${outdir}/${name}/evaluation.log"
}
