// The augmentation stage taken out of a wav.scp line.  The reference's scripts (steps/data/reverberate_data_dir.py:366, :220-232,
// :273-275, :291-294; steps/data/augment_data_dir_new.py:86-116) write entries such as
//   <source> | wav-reverberate --shift-output=true --impulse-response="sox rir.wav -r 8000 -t wav - |" - - |
//   wav-reverberate --shift-output=true --additive-signals='noise.wav wav-reverberate --duration=D - - |,...' --start-times='0,...'
//       --snrs='15,...' file.wav - |
// RecognizeWavPipeline takes such a line as text: a pipe whose LAST stage is wav-reverberate with only the options of the tool,
// reading "-" (the stages before it are the source) or one file, writing "-".  One level of nesting is taken inside
// --additive-signals: an element whose last stage is wav-reverberate with --duration and / or --impulse-response and nothing
// else.  Anything else - another option, --multi-channel-output, deeper nesting, a stage after the tool, unbalanced quotes,
// anything a shell would expand in the tool's own words - is not this pipeline and is run as a command, as before.
// compute-mfcc-feats then reads the source, the impulse response and the additive signals itself and reverberates on the device
// in the batch the MFCC is computed from (LoadWavJob, RunWavJobs), quantising to 16 bits in between exactly as the tool's
// output file would have been.  XVEC_DEBUG=fuse_wav=0 turns the recognition off.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/xvec_hip.h"

namespace xv {

struct FusedWavAdd;
struct FusedWav {
  std::string source;             // rxfilename of the input: a file, or "stage | stage |"
  xv_reverb_options opts;
  std::string impulse_response;   // rxfilename, "" = none
  std::vector<FusedWavAdd> add;
};
struct FusedWavAdd {
  std::string rx;                 // rxfilename of a plain additive signal (nested == false)
  bool nested = false;
  std::shared_ptr<FusedWav> inner;   // the nested wav-reverberate (no additive signals of its own)
  float snr = 0.f, start = 0.f;
};

bool RecognizeWavPipeline(const std::string& rxfilename, FusedWav* out);
// A text form for the tests: one "name=value" line per field.
std::string DescribeFusedWav(const FusedWav& p);

// One utterance read from its files, waiting for the device.  Host I/O and the tool's own checks (sampling rates, counts of the
// lists, channels) happen in LoadWavJob, which throws KioError with the tool's messages.
struct WavJob {
  int rate = 0;
  xv_reverb_options opts;
  std::vector<float> input, rir;
  struct Add {
    std::vector<float> samples;          // filled at once for a plain signal, by RunWavJobs for a nested one
    std::unique_ptr<WavJob> nested;
    float snr = 0.f, start = 0.f;
  };
  std::vector<Add> add;
  int64_t out_len = 0;                   // known after loading
  std::vector<int16_t> out;              // filled by RunWavJobs
  int64_t clipped = 0;
};
void LoadWavJob(const FusedWav& p, WavJob* job);
// Reverberates every job on the device: the nested ones first, then the jobs themselves, one launch sequence per set of equal
// options and rate.  A job's bytes do not depend on the others'.
void RunWavJobs(int device, const std::vector<WavJob*>& jobs);

}  // namespace xv
