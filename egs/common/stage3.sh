#!/usr/bin/env bash
# Stages 2 (token list generation) and 3 (network training) of the jatts recipes on the MI355X path.  Sourced by egs/*/tts*/run.sh with the
# reference's variables set: conf, dumpdir, train_set, dev_set, token_type, token_column, g2p, cleaner, nlsyms_txt, blank, oov, sos_eos, expdir,
# resume, verbose, n_gpus (reference egs/jsut/tts1/run.sh:66-76,166-218), and the same layout: the token list under
# ${dumpdir}/token_list/${train_set}_${token_type}[_${cleaner}][_${g2p}]/tokens.txt, and
# exp/<expname>/{config.yml,stats.npz,tokens.txt,checkpoint-*steps.pkl,train.log}.  Differences: the statistics are the .npz that stage 1 here writes
# (a reference-made stats.h5 next to it is copied too, for hosts with h5py), n_gpus > 1 is honoured (the reference logs "Not Implemented yet"; every rank starts from rank 0's parameters, jatts_amd.training.broadcast_model;
# this launcher line itself was not run on a multi-GPU node:
# one process per GPU under torch.distributed.run, as in stage4.sh), and train_precision / attention_precision / train_seed / resident_gb
# (recipe variables that every run.sh declares, empty unless the environment sets them, so --train_seed 0 works on the command line) are passed on as --precision / --attention-precision / --seed / --resident-gb when set.
# shellcheck disable=SC2154
stage2_tokens() {
    local token_listdir="${dumpdir}/token_list/${train_set}_${token_type}"
    [ "${cleaner}" != none ] && token_listdir+="_${cleaner}"
    [ "${token_type}" = phn ] && token_listdir+="_${g2p}"
    token_list="${token_listdir}/tokens.txt"
    mkdir -p "${token_listdir}"
    "${python}" -m jatts_amd.bin.generate_token_list \
        --csv "data/${train_set}.csv" \
        --out "${token_list}" \
        --column "${token_column}" \
        --non_linguistic_symbols "${nlsyms_txt:-none}" \
        --cleaner "${cleaner}" \
        --add_symbol "${blank:-<blank>}:0" \
        --add_symbol "${oov:-<unk>}:1" \
        --add_symbol "${sos_eos:-<sos/eos>}:-1" > "${token_listdir}/generate_token_list.log" 2>&1 || { tail -20 "${token_listdir}/generate_token_list.log"; exit 1; }
    log "Successfully finished token list generation."
}

stage3_train() {
    local token_listdir="${dumpdir}/token_list/${train_set}_${token_type}"
    [ "${cleaner}" != none ] && token_listdir+="_${cleaner}"
    [ "${token_type}" = phn ] && token_listdir+="_${g2p}"
    [ -e "${expdir}" ] || mkdir -p "${expdir}"
    local stats=""
    if [ -e "${dumpdir}/${train_set}/stats.npz" ]; then cp "${dumpdir}/${train_set}/stats.npz" "${expdir}/"; stats="${expdir}/stats.npz"; fi
    if [ -e "${dumpdir}/${train_set}/stats.h5" ]; then cp "${dumpdir}/${train_set}/stats.h5" "${expdir}/"; [ -n "${stats}" ] || stats="${expdir}/stats.h5"; fi
    [ -n "${stats}" ] || { log "${dumpdir}/${train_set}/stats.npz does not exist: run stage 1 first"; exit 1; }
    cp "${token_listdir}/tokens.txt" "${expdir}/tokens.txt"
    local launcher=("${python}" -m jatts_amd.bin.tts_train)
    if [ "${n_gpus}" -gt 1 ]; then
        launcher=("${python}" -m torch.distributed.run --nnodes=1 --nproc-per-node "${n_gpus}" --master-addr 127.0.0.1
                  --master-port "${master_port:-29517}" -m jatts_amd.bin.tts_train)
    fi
    log "Training start. See the progress via ${expdir}/train.log."
    "${launcher[@]}" \
        --config "${conf}" \
        --train-csv "data/${train_set}_raw_feat.csv" \
        --dev-csv "data/${dev_set}_raw_feat.csv" \
        --stats "${stats}" \
        --token-list "${expdir}/tokens.txt" \
        --token-column "${token_column}" \
        --outdir "${expdir}" \
        --resume "${resume:-}" \
        ${train_precision:+--precision "${train_precision}"} \
        ${attention_precision:+--attention-precision "${attention_precision}"} \
        ${train_seed:+--seed "${train_seed}"} \
        ${resident_gb:+--resident-gb "${resident_gb}"} \
        --verbose "${verbose}" > "${expdir}/train.log" 2>&1 || { tail -20 "${expdir}/train.log"; exit 1; }
    log "Successfully finished training."
}
