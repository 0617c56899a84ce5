#!/usr/bin/env bash
# Stage 1 (feature extraction and statistics) of the jatts recipes on the MI355X path.  Sourced by egs/*/tts*/run.sh with the
# reference's variables set: conf, dumpdir, train_set, dev_set, test_set, verbose (reference egs/jsut/tts2/run.sh:123-162), and the
# same layout: ${dumpdir}/<set>/feats/<sample_id>.npz, data/<set>_raw_feat.csv (data/<set>.csv plus a feat_path column),
# ${dumpdir}/${train_set}/stats.npz.  Differences: ONE GPU process per set does the whole csv in ragged batches (no csv split, no
# train_cmd, no background jobs), the test set is extracted too, and the dumps and the statistics are .npz (the format the later
# stages here read; tools/h5stats_to_npz.py goes the other way for a reference-made stats.h5).  A config that lists pitch (the
# FastSpeech2 ones) with pitch_extract_type: dio is refused by the CLI with its message: nothing is skipped silently.  With
# pitch_extract_type: acf the CLI extracts pitch with this package's own autocorrelation estimator (parity with DIO UNPINNED), reading
# the speakers' ranges from conf/f0.yaml where it exists.  Runs under the caller's set -euo pipefail:
# the first failing step ends the stage.
# shellcheck disable=SC2154
stage1_features() {
    local name
    for name in "${train_set}" "${dev_set}" "${test_set}"; do
        [ -e "data/${name}.csv" ] || { log "data/${name}.csv does not exist: stage 0 (data preparation) is the reference recipe's own"; exit 1; }
        mkdir -p "${dumpdir}/${name}/feats"
        cp "data/${name}.csv" "data/${name}_raw_feat.csv"
        log "Feature extraction start. See the progress via ${dumpdir}/${name}/preprocessing.log."
        local f0=()
        [ -e conf/f0.yaml ] && f0=(--f0_path conf/f0.yaml)
        "${python}" -m jatts_amd.bin.preprocess \
            --config "${conf}" \
            --csv "data/${name}_raw_feat.csv" \
            --dumpdir "${dumpdir}/${name}/feats" \
            "${f0[@]}" \
            --batch-size "${preprocess_batch_size:-32}" \
            --verbose "${verbose}" > "${dumpdir}/${name}/preprocessing.log" 2>&1 || { tail -20 "${dumpdir}/${name}/preprocessing.log"; exit 1; }
        log "Successfully finished feature extraction of ${name} set."
    done
    log "Successfully finished feature extraction."

    log "Statistics computation start. See the progress via ${dumpdir}/${train_set}/compute_statistics.log."
    "${python}" -m jatts_amd.bin.compute_statistics \
        --csv "data/${train_set}_raw_feat.csv" \
        --out "${dumpdir}/${train_set}/stats.npz" \
        --verbose "${verbose}" > "${dumpdir}/${train_set}/compute_statistics.log" 2>&1 || { tail -20 "${dumpdir}/${train_set}/compute_statistics.log"; exit 1; }
    log "Successfully finished calculation of statistics."
}
