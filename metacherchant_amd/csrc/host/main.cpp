// metacherchant -- native launcher of the MI355X tools.  Mirrors the command line of the reference (src/Runner.java, the launch
// options of itmo!/utils/tool/Tool.java:59-143 and every tool's own parameters: options.cpp) and its output surface (SURVEY.md
// Appendix D), and drives libmcgpu.so through the C ABI of include/mcgpu.h.  The tools are one unit each or a pair (tool_*.cpp) over
// what they share (cli.h, device.h); this unit says which options go with which tool and dispatches.
#include "cli.h"

using namespace mch;

namespace {

int run(const Options &o)
{
    if (o.compact_given && (o.tool == "kmer-counter" || o.tool == "environment-finder-multi"))  // (they share environment-finder's table)
        throw Error("--compact does not apply to --tool " + o.tool);
    if (o.trim_on_given && (o.tool == "kmer-counter" || o.tool == "environment-finder-multi")) throw Error("--trim-on does not apply to --tool " + o.tool);
    if (o.trim && o.trim_on == "gpu" && !o.devices.empty())  // (a group has no single context to run mc_trim_paths on)
        throw Error("--trim-on gpu does not go with --devices: the trim of a group's walk runs on the host (--trim-on host or auto)");
    if (o.join_given && o.tool != "environment-finder-multi") throw Error("--join does not apply to --tool " + o.tool);
    if (o.kmers_io_given && o.tool != "kmer-counter" && o.tool != "reads-classifier" && o.tool != "triple-reads-classifier")
        throw Error("--kmers-io does not apply to --tool " + o.tool);
    if (o.parse_given && o.tool != "reads-classifier" && o.tool != "triple-reads-classifier" && o.tool != "seq-cov" && o.tool != "fmt-visualizer" &&
        o.tool != "environment-assembler-finder")
        throw Error("--parse does not apply to --tool " + o.tool);
    if (o.render_given && o.tool != "reads-classifier" && o.tool != "triple-reads-classifier") throw Error("--render does not apply to --tool " + o.tool);
    if (o.tool == "kmer-counter") return run_kmer_counter(o);
    if (o.tool == "environment-finder-multi") return run_multi(o);
    if (o.tool == "reads-classifier") return run_reads_classifier(o);
    if (o.tool == "triple-reads-classifier") return run_triple_reads_classifier(o);
    if (o.tool == "seq-cov") return run_seq_cov(o);
    if (o.tool == "recipient-visualiser") return run_recipient_visualiser(o);
    if (o.tool == "environment-assembler-finder") return run_assembler_finder(o);
    if (o.tool == "fmt-visualizer") return run_fmt_visualizer(o);
    if (o.tool != "environment-finder")
        throw Error("Tool '" + o.tool + "' is not part of this build: only environment-finder, kmer-counter, environment-finder-multi, "
                    "reads-classifier, triple-reads-classifier, recipient-visualiser, environment-assembler-finder, fmt-visualizer and seq-cov are");
    return run_environment_finder(o);
}

}  // namespace

int main(int argc, char **argv)
{
    try {
        if (argc <= 1) { usage(); return 0; }
        const Options o = parse_args(argc, argv);
        if (o.help) { usage(); return 0; }
        return run(o);
    } catch (const std::exception &e) {
        logline("ERROR", e.what());
        return 1;  // System.exit(1) on ExecutionFailedException, itmo!/utils/tool/Tool.java:450-462
    }
}
