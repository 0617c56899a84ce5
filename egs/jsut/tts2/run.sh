#!/usr/bin/env bash
# egs/jsut/tts2 on the MI355X path: the reference recipe's interface (same variables, same --option syntax, same directory
# layout: exp/<expname>/{config.yml,stats.h5,tokens.txt,*.pkl} -> exp/<expname>/results/<checkpoint>/<set>/wav/*.wav) with
# stage 1 (feature extraction and statistics, egs/common/stage1.sh), stages 2 and 3 (token list and training, egs/common/stage3.sh) and stage 4
# (network decoding, egs/common/stage4.sh) and stage 5 (objective evaluation, egs/common/stage5.sh) running on jatts_amd.  Stages -1, 0 (download, data preparation) are the reference's
# and are not rebuilt here: run them there, or start this script inside the reference's recipe directory.
#     ./run.sh --stage 2 --stop_stage 3 [--conf conf/fastspeech2.v1.yaml] [--tag mytag] [--resume exp/.../checkpoint-10000steps.pkl] [--n_gpus 8]
#     ./run.sh --stage 1 --stop_stage 1 [--conf conf/matcha_tts.mas.v1.yaml] [--dumpdir dump]
#     ./run.sh --stage 4 --stop_stage 4 --tag mytag [--checkpoint exp/.../checkpoint-100000steps.pkl] [--n_gpus 8]

log() {
    local fname=${BASH_SOURCE[1]##*/}
    echo -e "$(date '+%Y-%m-%dT%H:%M:%S') (${fname}:${BASH_LINENO[0]}:${FUNCNAME[1]}) $*"
}

HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
REPO_ROOT="$(cd "${HERE}/../../.." && pwd)"
export PYTHONPATH="${REPO_ROOT}${PYTHONPATH:+:${PYTHONPATH}}"
export PYTHONIOENCODING=UTF-8
python=${PYTHON:-python3}

# basic settings (reference egs/jsut/tts2/run.sh:14-58)
stage=4        # stage to start
stop_stage=4   # stage to stop
verbose=1      # verbosity level (lower is less info)
n_gpus=1       # number of gpus (decoding: one process per GPU, utterances sharded)

conf=conf/matcha_tts.mas.v1.yaml

# feature extraction related setting (stage 1)
dumpdir=dump                # directory to dump full features
preprocess_batch_size=32    # utterances per ragged batch

# text related setting
token_type="phn"
token_column="phonemes"
g2p=pyopenjtalk
cleaner=none
oov="<unk>"            # Out of vocabulary symbol.
blank="<blank>"        # CTC blank symbol.
sos_eos="<sos/eos>"    # sos and eos symbols.
nlsyms_txt=none        # Non-linguistic symbol list (needed if existing).

# training related setting
tag=""         # tag for directory to save model
resume=""      # checkpoint path to resume training (e.g. <path>/<to>/checkpoint-10000steps.pkl)
train_precision=""    # the trainers' arithmetic (fp32 when empty; fp32_bf16x3 = f32 tensors, f32-equivalent emulated MFMA operands)
attention_precision="${attention_precision:-}"  # arithmetic of the attention products in training and decoding (fp32 | fp32_bf16x3; what the precision means when empty)
train_seed="${train_seed:-}"         # seed of the initial parameters and the shuffle (unseeded when empty, as the reference)
resident_gb="${resident_gb:-}"        # largest training set, in GiB, kept resident on the device (64 when empty)
expdir=""      # exp/<expname>; derived from conf / tag like the reference when empty

# decoding related setting
outdir=
checkpoint=""  # checkpoint path to be used for decoding; if not provided, the latest one will be used
precision=fp32        # fp32 = the reference's arithmetic; fp32_bf16x3 = f32 tensors, f32-equivalent emulated MFMA operands (1.35x; fp32_bf16x3_6p: 1.5x);
                      # fp32_split = f32 tensors + split-precision MFMA operands (2.5x); fp16 = fast mode
decode_batch_size=64  # utterances per ragged batch
master_port=29517

# evaluation related setting (stage 5)
eval_metrics=""       # metrics of stage 5; empty: what this package computes (mcd); asr and sheet are refused by name
eval_batch_size=16    # pairs per ragged batch

# shellcheck disable=SC1091
. "${REPO_ROOT}/egs/common/parse_options.sh" || exit 1
. "${REPO_ROOT}/egs/common/stage1.sh" || exit 1
. "${REPO_ROOT}/egs/common/stage3.sh" || exit 1
. "${REPO_ROOT}/egs/common/stage4.sh" || exit 1
. "${REPO_ROOT}/egs/common/stage5.sh" || exit 1

set -euo pipefail

train_set="train"
dev_set="dev"
test_set="test"

if [ -z "${expdir}" ]; then
    if [ -z "${tag}" ]; then
        expname="${train_set}_${token_type}_${cleaner}_$(basename "${conf%.*}")"
    else
        expname="${train_set}_${token_type}_${cleaner}_${tag}"
    fi
    expdir=exp/${expname}
fi

if [ "${stage}" -le 0 ]; then
    log "Stages <= 0 (download, data preparation) are the reference recipe's own: run them there."
fi

if [ "${stage}" -le 1 ] && [ "${stop_stage}" -ge 1 ]; then
    log "Stage 1: Feature extraction"
    stage1_features
fi

if [ "${stage}" -le 2 ] && [ "${stop_stage}" -ge 2 ]; then
    log "Stage 2: Token list generation"
    stage2_tokens
fi

if [ "${stage}" -le 3 ] && [ "${stop_stage}" -ge 3 ]; then
    log "Stage 3: Network training"
    stage3_train
fi

if [ "${stage}" -le 4 ] && [ "${stop_stage}" -ge 4 ]; then
    log "Stage 4: Network decoding"
    stage4_decode
fi

if [ "${stage}" -le 5 ] && [ "${stop_stage}" -ge 5 ]; then
    log "Stage 5: Objective evaluation"
    stage5_evaluate
fi
