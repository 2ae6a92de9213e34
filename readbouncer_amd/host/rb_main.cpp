// rb_main.cpp -- `readbouncer_amd --config file.toml`: the build and classify usages of ReadBouncer's CLI
// (src/main/main.cpp:274-406, src/main/parser.hpp:13-37, src/main/ibfbuild.hpp:21-180,
// src/main/classify.hpp:142-380) on top of the C++ mirror.  The chunk loop of classify_reads is run
// batch-wise: all reads of a batch are classified on chunk i in one GPU launch, reads that are still
// unclassified go on to chunk i+1 -- per read this is the reference's loop (classify.hpp:262-299).
// usage = "target" runs as an offline replay of the live classification step (pre-basecalled chunks from read_files
// through rb_live_*); the MinKNOW client, the basecallers and usage "test" (connection test) are out of scope.
#include <sys/resource.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "../../include/readbouncer_amd.hpp"
#include "../../include/readbouncer_amd_tuning.h"  // --calibrate only
#include "config_reader.hpp"
#include "seqio.hpp"

bool ConfigReader::filterException(std::filesystem::path& file) { return rb_is_ibf_file(file.string().c_str()) == 1; }

// plain-text stand-in for the reference's spdlog "ReadBouncerLog" (src/main/main.cpp:97): <log_directory>/ReadBouncerLog.txt
static std::ofstream g_log;
static void log_line(const std::string& level, const std::string& msg)
{
    if (g_log.is_open()) g_log << "[" << level << "] " << msg << std::endl;
}

// results struct of the reference's tests (classify.hpp:127-134)
struct ClassificationResults
{
    uint64_t found = 0;
    uint16_t failed = 0;
    uint64_t too_short = 0;
    uint64_t readCounter = 0;
} ClassificationResults_;

// build --write-bin-map: beside <name>.ibf, <name>.bins.tsv with one line per bin -- the fragment of which record it holds.  A bin is a
// fragment_size stretch of a reference record (src/IBF/IBFBuild.cpp:165-204), so the table turns the bin numbers of
// classify --report-bins into loci.  No counterpart in the reference.
static bool g_write_bin_map = false;
// the two head lines of every <name>.bins.tsv, whoever writes it (build --write-bin-map, --edit-ibf)
static void write_bin_map_head(std::ostream& out)
{
    out << "# start / end are positions in the record AFTER cutOutNNNs (every N removed): the sequence the reference fragments\n";
    out << "bin\trecord_id\tstart\tend\n";
}
static void write_bin_map(const std::string& path, const std::vector<interleave::RefSeq>& records, const interleave::IBFConfig& config)
{
    std::ofstream out(path);
    if (!out) throw std::runtime_error("Unable to open the file: " + path);
    write_bin_map_head(out);
    uint64_t bin = 0;
    std::vector<uint64_t> s, e;
    for (const interleave::RefSeq& r : records) {  // the records and the order of IBF::create_filter
        if (r.seq.size() < config.kmer_size) continue;
        std::string c(r.seq.size(), '\0');
        c.resize(rb_cut_out_nnns(r.seq.data(), r.seq.size(), &c[0]));
        const size_t n = rb_fragment_bounds(c.size(), config.fragment_length, config.kmer_size, config.overlap_length, nullptr, nullptr, 0);
        s.resize(n);
        e.resize(n);
        rb_fragment_bounds(c.size(), config.fragment_length, config.kmer_size, config.overlap_length, s.data(), e.data(), n);
        for (size_t i = 0; i < n; ++i) out << bin++ << '\t' << r.seqid << '\t' << s[i] << '\t' << e[i] << '\n';
    }
}

// --bin-map: the table above read back, ONE parser for both reports: bin -> "record_id\tstart\tend" ...
static std::vector<std::string> read_bin_map_rows(const std::string& path)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Unable to open the file: " + path);
    std::vector<std::string> rows;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#' || line.compare(0, 4, "bin\t") == 0) continue;
        const size_t a = line.find('\t'), b = a == std::string::npos ? a : line.find('\t', a + 1);
        if (b == std::string::npos) throw std::runtime_error("not a bin map: " + path);
        const size_t bin = (size_t)std::stoull(line.substr(0, a));
        if (bin >= rows.size()) rows.resize(bin + 1);
        rows[bin] = line.substr(a + 1);
    }
    return rows;
}
// ... and its first column alone (classify --report-bins): bin -> record id of one filter
static std::vector<std::string> read_bin_map(const std::string& path)
{
    std::vector<std::string> rec = read_bin_map_rows(path);
    for (std::string& r : rec) r.resize(std::min(r.size(), r.find('\t')));
    return rec;
}

// --filter-stats <file.ibf> / build --filter-stats: how full is each bin of the filter in HBM, and what false-positive rate does that mean?
// The reference sizes a filter for max_fp = 0.01 at fragment_size - k + 1 k-mers per bin (src/IBF/IBFConfig.hpp:77, IBFBuild.cpp:404-413) and
// nothing holds an updated or foreign filter to it.  One pass over the resident table (rb_dibf_bin_occupancy), a summary on stdout and
// <name>.binstats.tsv beside the filter: bin, bits, load, fpr, est_kmers and -- with a bin map of build --write-bin-map -- the record and
// fragment bounds of the bin.  Returns 0, or 3 when a bin's false-positive rate is over max_fp.
static bool g_filter_stats = false;
static double g_stats_max_fp = 0.01;        // --max-fp
static uint32_t g_stats_chunk_length = 360;  // --chunk-length: the read length the summary's noise floor is given for
static int filter_stats(interleave::IBF& filter, const std::string& ibf_path, const std::string& bin_map_path, double error_rate)
{
    const interleave::IBF::BinOccupancy occ = filter.bin_occupancy(g_stats_max_fp);
    const rb_bin_occupancy_summary& s = occ.summary;
    const size_t n = occ.bits.size();
    std::vector<double> load(n), fpr(n), est(n);
    interleave::throw_status(rb_bin_occupancy_derive(occ.bits.data(), n, s.n_blocks, s.n_hash, load.data(), fpr.data(), est.data()),
                             "rb_bin_occupancy_derive");
    const std::vector<std::string> map_rows = bin_map_path.empty() ? std::vector<std::string>() : read_bin_map_rows(bin_map_path);
    std::filesystem::path out_path(ibf_path);
    out_path.replace_extension("binstats.tsv");
    std::ofstream out(out_path);
    if (!out) throw std::runtime_error("Unable to open the file: " + out_path.string());
    out << std::setprecision(17);
    out << "bin\tbits\tload\tfpr\test_kmers" << (bin_map_path.empty() ? "" : "\trecord_id\tstart\tend") << '\n';
    for (size_t j = 0; j < n; ++j) {
        out << j << '\t' << occ.bits[j] << '\t' << load[j] << '\t' << fpr[j] << '\t' << est[j];
        if (!bin_map_path.empty()) out << '\t' << (j < map_rows.size() && !map_rows[j].empty() ? map_rows[j] : std::string("\t\t"));
        out << '\n';
    }
    out.close();
    if (!out) throw std::runtime_error("short write to " + out_path.string());
    const uint64_t kmer_size = filter.getFilter().kmerSize;
    const uint64_t n_kmers = g_stats_chunk_length >= kmer_size ? g_stats_chunk_length - kmer_size + 1 : 0;
    std::cout << "FILTER_STATS file=" << ibf_path << " bins=" << s.n_bins << " blocks=" << s.n_blocks << " hash_functions=" << s.n_hash
              << " bits_total=" << s.bits_total << " empty_bins=" << s.empty_bins << "\n"
              << "  load   mean=" << s.mean_load << " max=" << s.max_load << " (over the non-empty bins)\n"
              << "  fpr    mean=" << s.mean_fpr << " max=" << s.max_fpr << " max_fp=" << g_stats_max_fp << "\n"
              << "  fullest_bin=" << s.max_bin << " bits=" << s.max_bits << " emptiest_bin=" << s.min_bin << " bits=" << s.min_bits << "\n"
              << "  bins_over_max_fp=" << s.bins_over_max_fp << "\n"
              << "  chunk_length=" << g_stats_chunk_length << " threshold=" << rb_threshold(g_stats_chunk_length, kmer_size, error_rate, 0.95)
              << " at error_rate=" << error_rate << "; expected false-positive hits in the fullest bin=" << (double)n_kmers * s.max_fpr << "\n"
              << "  written " << out_path.string() << std::endl;
    return s.bins_over_max_fp ? 3 : 0;
}

// --edit-ibf <a.ibf> [--with <b.ibf> ...] --output <out.ibf> with one of --plan / --merge-every / --drop-records: a new filter whose bins are
// ORs of bins of the loaded ones (rb_dibf_assemble) -- drop a record, merge fragments into coarser bins, join filters -- without the FASTA.
// The reference only appends (IBF::update_filter, src/IBF/IBFBuild.cpp:223-321).  The plan is a list of (filter, bin) per out bin, filter
// 0 = --edit-ibf, the --with files follow in order.
struct EditOptions
{
    std::string input, output, plan_path, drop_records;
    std::vector<std::string> with;
    uint64_t merge_every = 0;
    bool merge_given = false;
};
static std::vector<std::string> split_commas(const std::string& list)
{
    std::vector<std::string> out;
    size_t pos = 0;
    while (pos <= list.size()) {
        const size_t comma = list.find(',', pos);
        const std::string tok = list.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
        if (!tok.empty()) out.push_back(tok);
        if (comma == std::string::npos) break;
        pos = comma + 1;
    }
    return out;
}
// rows `out_bin<TAB>filter<TAB>bin`; `#` starts a comment; `# bins=N` fixes the bin count, otherwise it is the highest out bin + 1
static std::vector<std::vector<rb_bin_ref>> read_plan(const std::string& path)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Unable to open the file: " + path);
    struct Row { uint64_t out_bin; rb_bin_ref ref; size_t line_no; };
    std::vector<Row> rows;  // the plan is sized only when every row has been read and held against `# bins=N`
    uint64_t fixed = 0, highest = 0;
    bool have_fixed = false;
    std::string line;
    size_t line_no = 0;
    while (std::getline(in, line)) {
        ++line_no;
        const std::string where = path + ":" + std::to_string(line_no) + ": ";
        const size_t hash = line.find('#');
        if (hash != std::string::npos) {
            const size_t b = line.find("bins=", hash);
            if (line.find_first_not_of(" \t") == hash && b != std::string::npos && line.find_first_not_of(" \t", hash + 1) == b) {
                char* end = nullptr;
                const unsigned long long v = std::strtoull(line.c_str() + b + 5, &end, 10);
                if (end == line.c_str() + b + 5 || v == 0 || v >= (1ull << 31)) throw std::runtime_error(where + "malformed bins=N");
                fixed = v;
                have_fixed = true;
            }
            line.resize(hash);
        }
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        unsigned long long v[3];
        const char* p = line.c_str();
        for (int i = 0; i < 3; ++i) {
            while (*p == ' ' || *p == '\t') ++p;
            char* end = nullptr;
            if (*p < '0' || *p > '9') throw std::runtime_error(where + "malformed plan row (out_bin<TAB>filter<TAB>bin)");
            v[i] = std::strtoull(p, &end, 10);
            p = end;
        }
        while (*p == ' ' || *p == '\t' || *p == '\r') ++p;
        if (*p != '\0') throw std::runtime_error(where + "malformed plan row (out_bin<TAB>filter<TAB>bin)");
        if (v[0] >= (1ull << 31) || v[1] > 0xFFFFFFFFull || v[2] > 0xFFFFFFFFull) throw std::runtime_error(where + "plan row out of range");
        rows.push_back(Row{v[0], rb_bin_ref{(uint32_t)v[1], (uint32_t)v[2]}, line_no});
        highest = std::max<uint64_t>(highest, v[0]);
    }
    if (have_fixed)
        for (const Row& r : rows)
            if (r.out_bin >= fixed)
                throw std::runtime_error(path + ":" + std::to_string(r.line_no) + ": plan row out of range: out bin " + std::to_string(r.out_bin) + " with bins=" + std::to_string(fixed));
    if (!have_fixed && rows.empty()) throw std::runtime_error(path + ": the plan has no out bin");
    // without `# bins=N` the bin count is the highest out bin + 1: a number far beyond what the rows could fill is a typo, not a plan
    if (!have_fixed && highest >= (1ull << 24) && highest >= 1024 * (uint64_t)rows.size())
        throw std::runtime_error(path + ": plan row out of range: out bin " + std::to_string(highest) + " with " + std::to_string(rows.size()) + " rows and no `# bins=N` line");
    std::vector<std::vector<rb_bin_ref>> plan(have_fixed ? fixed : highest + 1);
    for (const Row& r : rows) plan[r.out_bin].push_back(r.ref);
    return plan;
}
static int edit_ibf(const EditOptions& eo, const std::vector<std::string>& bin_map_args, int device, bool with_stats, double error_rate)
{
    if (eo.output.empty()) throw std::runtime_error("--edit-ibf needs --output <out.ibf>");
    if ((eo.plan_path.empty() ? 0 : 1) + (eo.merge_given ? 1 : 0) + (eo.drop_records.empty() ? 0 : 1) != 1)
        throw std::runtime_error("--edit-ibf needs exactly one of --plan <plan.tsv>, --merge-every N, --drop-records id[,id...]");
    std::vector<std::string> map_paths;
    for (const std::string& a : bin_map_args)
        for (const std::string& m : split_commas(a)) map_paths.push_back(m);
    std::vector<std::string> paths{eo.input};
    paths.insert(paths.end(), eo.with.begin(), eo.with.end());
    if (paths.size() > RB_ASSEMBLE_MAX_SOURCES) throw std::runtime_error("--edit-ibf: at most " + std::to_string(RB_ASSEMBLE_MAX_SOURCES) + " filters");
    if (!map_paths.empty() && map_paths.size() != paths.size())
        throw std::runtime_error("--bin-map: " + std::to_string(map_paths.size()) + " bin maps for " + std::to_string(paths.size()) + " filters");
    if (eo.merge_given && (eo.merge_every == 0 || paths.size() != 1)) throw std::runtime_error("--merge-every N: N >= 1, one filter only");
    if (!eo.drop_records.empty() && map_paths.empty()) throw std::runtime_error("--drop-records needs --bin-map");
    std::vector<interleave::TIbf> sources;
    uint64_t bins_in = 0;
    for (const std::string& p : paths) {
        interleave::IBFConfig cfg{};
        cfg.input_filter_file = p;
        cfg.device = device;
        interleave::IBF f{};
        f.load_filter(cfg);
        sources.push_back(f.getFilter());
        bins_in += sources.back().noOfBins;
    }
    std::vector<std::vector<std::string>> maps;  // per source: bin -> "record_id\tstart\tend"
    for (const std::string& m : map_paths) maps.push_back(read_bin_map_rows(m));
    auto record_of = [&](const rb_bin_ref& r) {
        if (r.filter >= maps.size() || r.bin >= maps[r.filter].size()) return std::string();
        const std::string& row = maps[r.filter][r.bin];
        return row.substr(0, row.find('\t'));
    };
    std::vector<std::vector<rb_bin_ref>> plan;
    if (!eo.plan_path.empty()) plan = read_plan(eo.plan_path);
    else if (eo.merge_given) {
        for (uint64_t j = 0; j < sources[0].noOfBins; j += eo.merge_every) {
            plan.emplace_back();
            for (uint64_t b = j; b < std::min<uint64_t>(j + eo.merge_every, sources[0].noOfBins); ++b) plan.back().push_back(rb_bin_ref{0u, (uint32_t)b});
        }
    } else {
        const std::vector<std::string> drop = split_commas(eo.drop_records);
        std::vector<bool> seen(drop.size(), false);
        for (uint32_t f = 0; f < sources.size(); ++f)
            for (uint64_t b = 0; b < sources[f].noOfBins; ++b) {
                const rb_bin_ref r{f, (uint32_t)b};
                const std::string rec = record_of(r);
                bool dropped = false;
                for (size_t d = 0; d < drop.size(); ++d)
                    if (!rec.empty() && rec == drop[d]) dropped = seen[d] = true;
                if (!dropped) plan.push_back(std::vector<rb_bin_ref>{r});
            }
        for (size_t d = 0; d < drop.size(); ++d)
            if (!seen[d]) throw std::runtime_error("--drop-records: no bin of record " + drop[d]);
        if (drop.empty()) throw std::runtime_error("--drop-records: no record id given");
        if (plan.empty()) throw std::runtime_error("--drop-records: no bin is left");
    }
    uint64_t n_refs = 0;
    for (const auto& l : plan) n_refs += l.size();
    interleave::IBF result{};
    result.assemble(sources, plan);
    const double kernel_s = rb_assemble_last_seconds();
    try {
        result.getFilter().store(eo.output);
    } catch (const interleave::IBFBuildException& e) {
        throw std::runtime_error("Could not store IBF to " + eo.output + ": " + e.what());
    }
    std::filesystem::path map_out(eo.output);
    map_out.replace_extension("bins.tsv");
    if (!maps.empty()) {
        std::ofstream out(map_out);
        if (!out) throw std::runtime_error("Unable to open the file: " + map_out.string());
        write_bin_map_head(out);
        for (size_t j = 0; j < plan.size(); ++j) {
            if (plan[j].empty()) continue;
            std::vector<std::string> ids;
            uint64_t lo = UINT64_MAX, hi = 0;
            bool bounds = true;
            for (const rb_bin_ref& r : plan[j]) {
                const std::string rec = record_of(r);
                if (std::find(ids.begin(), ids.end(), rec) == ids.end()) ids.push_back(rec);
                const std::string& row = maps[r.filter].size() > r.bin ? maps[r.filter][r.bin] : std::string();
                const size_t a = row.find('\t'), b = a == std::string::npos ? a : row.find('\t', a + 1);
                if (b == std::string::npos || b + 1 >= row.size() || a + 1 == b) { bounds = false; continue; }
                lo = std::min<uint64_t>(lo, std::stoull(row.substr(a + 1, b - a - 1)));
                hi = std::max<uint64_t>(hi, std::stoull(row.substr(b + 1)));
            }
            out << j << '\t';
            for (size_t i = 0; i < ids.size(); ++i) out << (i ? "," : "") << ids[i];
            if (ids.size() == 1 && bounds) out << '\t' << lo << '\t' << hi << '\n';
            else out << "\t\t\n";
        }
        out.close();
        if (!out) throw std::runtime_error("short write to " + map_out.string());
    }
    std::cout << "EDIT_IBF sources=" << sources.size() << " bins_in=" << bins_in << " bins_out=" << plan.size() << " refs=" << n_refs
              << " kernel_seconds=" << kernel_s << " output=" << eo.output << std::endl;
    if (with_stats) return filter_stats(result, eo.output, maps.empty() ? std::string() : map_out.string(), error_rate);
    return 0;
}

// buildIBF, src/main/ibfbuild.hpp:21-59
static interleave::TIbf buildIBF(ConfigReader config_reader, const std::string reference_file,
                                 const std::string bloom_filter_output_path)
{
    interleave::IBFConfig config{};
    config.reference_files.emplace_back(reference_file);
    config.output_filter_file = bloom_filter_output_path;
    config.kmer_size = (uint16_t)config_reader.IBF_Parsed.size_k;
    config.threads_build = (uint16_t)config_reader.IBF_Parsed.threads;
    config.fragment_length = (uint64_t)config_reader.IBF_Parsed.fragment_size;
    const auto t_parse = std::chrono::steady_clock::now();
    seqio::Reader in(reference_file);
    if (!in.is_open()) throw interleave::FileParserException("Unable to open the file: " + reference_file);
    std::vector<interleave::RefSeq> records;
    std::string id, seq;
    try {
        while (in.read_record(id, seq)) records.push_back({id.substr(0, id.find(' ')), seq});
    } catch (const std::exception& e) {
        throw interleave::FileParserException("ERROR: Problems parsing the file: " + reference_file + "[" + e.what() + "]");
    }
    const double parse_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_parse).count();
    interleave::IBF filter{};
    const auto t0 = std::chrono::steady_clock::now();
    interleave::FilterStats stats = filter.create_filter(config, records);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (g_write_bin_map) {
        std::filesystem::path map_path(bloom_filter_output_path);
        map_path.replace_extension("bins.tsv");
        write_bin_map(map_path.string(), records, config);
    }
    if (g_filter_stats) {  // from the table while it is still in HBM
        std::filesystem::path map_path(bloom_filter_output_path);
        map_path.replace_extension("bins.tsv");
        filter_stats(filter, bloom_filter_output_path, g_write_bin_map ? map_path.string() : std::string(), config_reader.IBF_Parsed.error_rate);
    }
    // where a build's time goes (profiles/cli_build.py reads this line): parsing the FASTA, cutOutNNNs + sizing, the filter's allocation
    // in HBM, the concatenation, rb_dibf_insert (H2D + the insert kernel), download + file
    std::cout << "BUILD_PHASES file=" << reference_file << " parse_s=" << parse_s << " load_seq_s=" << stats.timeLoadSeq
              << " alloc_filter_s=" << stats.timeAllocFilter << " concat_s=" << stats.timeConcat << " insert_s=" << stats.timeInsert
              << " save_s=" << stats.timeSaveFilter << " create_filter_s=" << stats.timeIBF << " bins=" << stats.totalBinsFile
              << " bases=" << stats.sumSeqLen << std::endl;
    const uint64_t validSeqs = stats.totalSeqsFile - stats.invalidSeqs;
    std::cerr << "IBF-build processed " << validSeqs << " sequences (" << stats.sumSeqLen / 1000000.0 << " Mbp) in " << secs
              << " seconds" << std::endl;
    if (stats.invalidSeqs > 0) std::cerr << " - " << stats.invalidSeqs << " invalid sequences were skipped" << std::endl;
    std::cerr << " - " << validSeqs << " sequences in " << stats.totalBinsFile + stats.newBins
              << " bins were written to the IBF" << std::endl;
    return filter.getFilter();
}

// getIBF, src/main/ibfbuild.hpp:69-180: load the file if it is an IBF, else build one from the FASTA.  Filters that only have
// to be LOADED are read and sent to the GPU side by side (a thread each: four 10-20 MB filters cost the time of one, part of every
// run's fixed cost); a list with a FASTA in it is worked through in order like the reference's.  The messages keep the list's order.
static std::vector<interleave::IBFMeta> getIBF(ConfigReader config, bool depleteFilter, bool targetFilter)
{
    const std::vector<std::filesystem::path>& files =
        depleteFilter ? config.IBF_Parsed.deplete_files : (targetFilter ? config.IBF_Parsed.target_files : std::vector<std::filesystem::path>{});
    struct Loaded { interleave::IBFMeta meta; std::string message; std::exception_ptr error; };
    std::vector<Loaded> loaded(files.size());
    bool all_ibf = files.size() > 1;
    for (std::filesystem::path file : files) all_ibf = all_ibf && config.filterException(file);
    auto load_one = [&](size_t i) {
        try {
            std::filesystem::path file = files[i];
            interleave::IBFMeta& filter = loaded[i].meta;
            filter.name = file.stem().string();
            if (config.filterException(file)) {
                interleave::IBF tf{};
                interleave::IBFConfig cfg{};
                cfg.input_filter_file = file.string();
                const auto t0 = std::chrono::steady_clock::now();
                interleave::FilterStats stats = tf.load_filter(cfg);
                filter.filter = tf.getFilter();
                loaded[i].message = std::to_string(stats.totalBinsFile) + " bins were loaded in " +
                                    std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()) +
                                    " seconds from the IBF";
            } else {
                std::filesystem::path out_path = std::filesystem::path(config.output_dir);
                out_path /= file.filename();
                out_path.replace_extension("ibf");
                filter.filter = buildIBF(config, file.string(), out_path.string());
            }
        } catch (...) {
            loaded[i].error = std::current_exception();
        }
    };
    if (all_ibf) {
        std::vector<std::thread> th;
        for (size_t i = 0; i < files.size(); ++i) th.emplace_back(load_one, i);
        for (std::thread& t : th) t.join();
    } else {
        for (size_t i = 0; i < files.size(); ++i) load_one(i);
    }
    std::vector<interleave::IBFMeta> out;
    for (Loaded& l : loaded) {
        if (l.error) std::rethrow_exception(l.error);
        if (!l.message.empty()) std::cerr << l.message << std::endl;
        out.emplace_back(std::move(l.meta));
    }
    return out;
}

// --verify-ibf: does this .ibf hold exactly what the reference fragmenter + insertKmer put there for this FASTA?  The
// first thing to run on a filter written by the reference itself: the hash and layout constants of the IBF are restated
// from SeqAn (readbouncer_amd/csrc/ibf_spec.h), and a file is where a wrong one would first show.
static int verify_ibf(const std::string& ibf_path, const std::string& fasta_path, uint64_t fragment_size)
{
    seqio::Reader in(fasta_path);
    if (!in.is_open()) { std::cerr << "ERROR: Unable to open the file: " << fasta_path << std::endl; return 1; }
    std::vector<interleave::RefSeq> records;
    std::string id, seq;
    while (in.read_record(id, seq)) records.push_back({id.substr(0, id.find(' ')), seq});
    interleave::IBFConfig cfg{};
    cfg.input_filter_file = ibf_path;
    cfg.fragment_length = fragment_size;
    interleave::IBF f{};
    interleave::IBF::VerifyReport rep = f.verify_filter(cfg, records);
    if (!rep.warning.empty()) std::cout << "WARNING: " << rep.warning << std::endl;
    const double load = rep.bits.payload_bits ? (double)rep.bits.file_bits / (double)rep.bits.payload_bits : 0.0;
    std::cout << "VERIFY file=" << ibf_path << " kmer_size=" << cfg.kmer_size << " bins_file=" << rep.bins_file
              << " bins_expected=" << rep.bins_expected << " file_bits=" << rep.bits.file_bits
              << " rebuilt_bits=" << rep.bits.rebuilt_bits << " new_bits=" << rep.bits.new_bits
              << " explained=" << (rep.bits.file_bits ? (double)(rep.bits.rebuilt_bits - rep.bits.new_bits) / (double)rep.bits.file_bits : 0.0)
              << " load=" << load << std::endl;
    if (rep.ok()) {
        std::cout << "VERIFY OK: re-inserting " << records.size() << " sequences sets no new bit" << std::endl;
        return 0;
    }
    if (rep.bins_file != rep.bins_expected)
        std::cout << "VERIFY FAILED: the file has " << rep.bins_file << " bins, these sequences at fragment_size " << fragment_size
                  << " make " << rep.bins_expected << " (wrong FASTA or fragment size?)" << std::endl;
    else
        std::cout << "VERIFY FAILED: " << rep.bits.new_bits << " of " << rep.bits.rebuilt_bits
                  << " re-inserted bits are clear in the file -- hash/layout constants (ibf_spec.h) or k-mer encoding differ" << std::endl;
    return 3;
}

// (seqan::Dna5String) of a character, printed back: ACGT in either case -> upper case, U/u -> T, everything else -> N
static const struct Dna5CharTable {
    char t[256];
    Dna5CharTable()
    {
        for (int c = 0; c < 256; ++c) t[c] = 'N';
        t['A'] = t['a'] = 'A'; t['C'] = t['c'] = 'C'; t['G'] = t['g'] = 'G'; t['T'] = t['t'] = 'T'; t['U'] = t['u'] = 'T';
    }
    char operator[](unsigned char c) const { return t[c]; }
} kDna5Char;

// n bytes of a read through that table.  unclassified.fasta is most of what a depletion run writes (every read that is
// not a target), so the table walk is given a 32-bytes-at-a-time form where the CPU has AVX2: fold case (c & 0xDF),
// compare with A C G T U, blend.
#if defined(__x86_64__) && defined(__GNUC__)
#include <immintrin.h>
__attribute__((target("avx2"))) static void dna5_map_avx2(char* dst, const char* src, size_t n)
{
    const __m256i fold = _mm256_set1_epi8((char)0xDF), cA = _mm256_set1_epi8('A'), cC = _mm256_set1_epi8('C'),
                  cG = _mm256_set1_epi8('G'), cT = _mm256_set1_epi8('T'), cU = _mm256_set1_epi8('U'), cN = _mm256_set1_epi8('N');
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        const __m256i v = _mm256_and_si256(_mm256_loadu_si256((const __m256i*)(src + i)), fold);
        const __m256i isU = _mm256_cmpeq_epi8(v, cU);
        const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, cA), _mm256_cmpeq_epi8(v, cC)),
                                           _mm256_or_si256(_mm256_cmpeq_epi8(v, cG), _mm256_cmpeq_epi8(v, cT)));
        __m256i r = _mm256_blendv_epi8(cN, v, ok);
        r = _mm256_blendv_epi8(r, cT, isU);
        _mm256_storeu_si256((__m256i*)(dst + i), r);
    }
    for (; i < n; ++i) dst[i] = kDna5Char[(unsigned char)src[i]];
}
static const bool kHaveAvx2 = __builtin_cpu_supports("avx2");
#else
static const bool kHaveAvx2 = false;
static void dna5_map_avx2(char*, const char*, size_t) {}
#endif
static inline void dna5_map(char* dst, const char* src, size_t n)
{
    if (kHaveAvx2) { dna5_map_avx2(dst, src, n); return; }
    for (size_t i = 0; i < n; ++i) dst[i] = kDna5Char[(unsigned char)src[i]];
}

struct ReadState
{
    bool classified = false, failed = false;
    int best = -1;
    std::string bin_rows;  // --report-bins: this read's lines of classified_bins.tsv
    std::string hit_rows;  // --report-hits: this read's lines of classified_hits.tsv
    std::string span_rows; // --report-spans: this read's lines of classified_spans.tsv
    std::string prefix_row; // --report-prefixes: this read's line of classified_prefixes.tsv
};

// --report-prefixes, per checkpoint: reads that reach it, reads with decision 0 / 1 / 2 there (a row that is not RB_OK has decision 0), reads
// first decided there, reads whose decision differs from the checkpoint before
constexpr size_t kPrefixTallies = 6;

// host pipeline knobs (command line)
struct IngestOptions
{
    size_t batch_reads = 65536;  // most reads per GPU call
    unsigned threads = 6;        // parser threads (one does ~3 GB/s of 250 bp FASTQ records)
    unsigned classify_threads = 0;  // threads running the chunk loop on the GPU and formatting their segment's output (one engine
                                    // each); 0 = [IBF] threads when the TOML sets it above 1 (the reference's meaning of that key:
                                    // classification threads, adaptive_sampling.hpp:745), else 4: since the engines of a device share
                                    // the merged copy of their filters the GPU side of a segment is short, and what a fifth and sixth
                                    // thread add is contention among the formatters (profiles/r04/cli_classifier_threads_*.txt, README
                                    // shape, M reads/s in-process with 4 / 5 / 6 threads: 23.8 / 21.9 / 21.2 on 16 M reads, 29.6 / 31.6 /
                                    // 28.0 on 64 M)
    bool calibrate = false;      // --calibrate: every classifier thread's engine fits the windows of its clock-phased gathers to this device first
                                 // (rb_engine_calibrate, one engine after the other: ~30 ms each; pays on long runs over narrow filters)
    bool mmap_output = false;    // --mmap-output: the classifier threads write the outputs through shared mappings of the files instead of
                                 // positional writes of a small buffer each (measured slower on tmpfs: page faults on fresh page-cache pages)
    size_t segment_mb = 32;      // file bytes per parsed segment (one GPU call of ~65 k reads of 250 bp; the page-locked staging blocks scale with it)
    size_t segment_bytes = 0;    // tests: segments far smaller than a megabyte (0 = segment_mb)
    size_t live_batch = 64;      // usage "target" replay: chunks per micro-batch
    bool report_bins = false;    // --report-bins: locate the reads every chunk classified (rb_locate_batch) and write classified_bins.tsv
    bool report_hits = false;    // --report-hits: list every (bin, strand) those reads hit (rb_hits_batch): classified_hits.tsv and bin_profile.tsv
    bool report_spans = false;   // --report-spans: where along those reads the best bin of every matching filter matched (rb_spans_batch): classified_spans.tsv
    bool report_prefixes = false;  // --report-prefixes: the decision of EVERY read at every prefix checkpoint (rb_prefix_batch): classified_prefixes.tsv, prefix_summary.tsv
    std::vector<uint32_t> prefix_lens;  // ... the checkpoints in bases, strictly rising (--prefix-lens a,b,c, or made from --prefix-step / --prefix-count)
    uint32_t prefix_step = 0, prefix_count = 0;
    uint32_t max_hits = 64;      // --max-hits N: records kept per (read, filter); n_hits in the report stays exact
    int pass_lists = RB_PASS_LISTS_CURRENT;  // --pass-lists off|current|build: --report-bins / --report-hits from a filter's list table
                                             // (rb_engine_set_pass_lists): where it has one, or building one; the files are the same bytes
    int wide_lists = RB_PASS_LISTS_OFF;      // --wide-lists off|current|build: classify counts filters of 8193 to 32 256 bins from their wide
                                             // list table (rb_engine_set_wide_lists); the files are the same bytes
    int wide_pass_lists = RB_PASS_LISTS_CURRENT;  // --wide-pass-lists off|current|build: --report-bins / --report-hits from such a filter's wide
                                             // list table (rb_engine_set_wide_pass_lists) where it has one -- one exists only if the run asked for it
                                             // with --wide-lists build -- or building one; the files are the same bytes
    int prefix_lists = RB_PASS_LISTS_OFF;    // --prefix-lists off|current|build: --report-prefixes from a filter's list table
                                             // (rb_engine_set_prefix_lists); the files are the same bytes
    int wide_prefix_lists = RB_PASS_LISTS_OFF;  // --wide-prefix-lists off|current|build: --report-prefixes from a wide list table
                                             // (rb_engine_set_wide_prefix_lists), filters of 8193 to 32256 bins; the files are the same bytes
    std::vector<std::string> bin_maps;  // --bin-map FILE (may repeat): <filter name>.bins.tsv of build --write-bin-map -> a record_id column
    size_t bytes() const { return segment_bytes ? segment_bytes : (segment_mb << 20); }
};

// what a classified segment adds to the outputs: exact byte counts per output file (target files first, unclassified.fasta last)
// -- known before a byte is formatted, so that the files can be laid out in read order while the formatting itself runs in
// parallel -- and the tallies of the segment
struct SegmentOutput
{
    std::vector<uint64_t> bytes;         // one per target file, unclassified.fasta last
    std::vector<uint64_t> per_target;    // IBFMeta.classified increments (classify.hpp:80,288)
    std::vector<std::string> error_lines;
    uint64_t found = 0, failed = 0;
};

// classify_reads, src/main/classify.hpp:142-380, as a pipeline: parser threads cut the memory-mapped read file into
// segments and stage the first chunk of every read (seqio::ParallelReader); classifier threads take the segments in file
// order, run the chunk loop on the GPU (one engine each: while one waits for the GPU the others prepare and format), size
// their segment's share of every output file, reserve it in file order (seqio::OrderedOutput) and then format the FASTA
// text straight into the files' page cache, all of them at once -- outputs byte-identical to a serial run.
static void classify_reads(ConfigReader& config, std::vector<interleave::IBFMeta> DepletionFilters,
                           std::vector<interleave::IBFMeta> TargetFilters, const IngestOptions& opt,
                           const std::vector<int>& devices)
{
    interleave::ClassifyConfig Conf{};
    std::unique_ptr<interleave::MultiDeviceClassifier> multi;
    if (devices.size() > 1 && (!DepletionFilters.empty() || !TargetFilters.empty()))
        multi.reset(new interleave::MultiDeviceClassifier(devices, DepletionFilters, TargetFilters));
    const bool deplete = DepletionFilters.size() >= 1, target = TargetFilters.size() >= 1;
    if (!deplete && !target) {
        std::cerr << "[Error] No depletion or target filters have been provided for classification! " << '\n';
        exit(1);
    }
    for (std::filesystem::path read_file : config.IBF_Parsed.read_files) {
        Conf.strata_filter = (uint16_t)-1;
        Conf.significance = 0.95;
        Conf.error_rate = config.IBF_Parsed.error_rate;
        uint64_t found = 0, too_short = 0, readCounter = 0;
        uint16_t failed = 0;
        double classify_seconds = 0.0;
        uint64_t classify_reads_n = 0;
        const auto wall0 = std::chrono::steady_clock::now();

        const size_t n_out = TargetFilters.size() + 1;  // <target>.fasta ..., unclassified.fasta last
        std::vector<std::unique_ptr<seqio::OrderedOutput>> outputs;
        for (size_t i = 0; i < n_out; ++i) {
            std::filesystem::path outfile(config.output_dir);
            outfile /= i < TargetFilters.size() ? TargetFilters[i].name + ".fasta" : std::string("unclassified.fasta");
            outputs.emplace_back(new seqio::OrderedOutput());
            const bool opened = outputs.back()->open(outfile.string(), opt.mmap_output);
            if (!opened && i + 1 == n_out) {  // (the reference checks unclassified.fasta only, classify.hpp:205-211)
                std::cerr << "ERROR: Unable to open the file: " << outfile.string() << std::endl;
                return;
            }
        }
        // --report-bins: <output_directory>/classified_bins.tsv, one line per (classified read, filter that matched it), in file order
        std::ofstream bins_out;
        std::vector<const interleave::IBFMeta*> all_filters;
        std::vector<std::vector<std::string>> bin_records;  // per filter: bin -> record id (empty: no map given)
        // --report-hits: classified_hits.tsv, one line per (bin, strand) such a read hit, in file order, and bin_profile.tsv, the number of
        // those reads that hit each bin over the whole run
        std::ofstream hits_out;
        std::vector<uint64_t> bin_profile;  // one entry per bin of every filter, filter after filter (rb_hits_out.bin_reads)
        // --report-spans: classified_spans.tsv, one line per (classified read, filter that matched it), in file order: where along the read the
        // locate pass's best bin matched on its best strand, positions in the read's coordinates
        std::ofstream spans_out;
        // --report-prefixes: classified_prefixes.tsv, one line per read of the run in file order -- per checkpoint the bases the row stands for,
        // the decision of the run's mode on that prefix, the best target and every filter's maximum -- and prefix_summary.tsv, per checkpoint
        // the tallies below over the whole run
        std::ofstream prefixes_out;
        const size_t n_cp = opt.report_prefixes ? opt.prefix_lens.size() : 0;
        std::vector<uint64_t> prefix_tally(n_cp * kPrefixTallies, 0);
        if (opt.report_bins || opt.report_hits || opt.report_spans || opt.report_prefixes) {
            if (multi) throw std::runtime_error("--report-bins, --report-hits, --report-spans and --report-prefixes work on one device");
            for (const interleave::IBFMeta& f : DepletionFilters) all_filters.push_back(&f);
            for (const interleave::IBFMeta& f : TargetFilters) all_filters.push_back(&f);
            bin_records.resize(all_filters.size());
            for (const std::string& path : opt.bin_maps) {
                std::string stem = std::filesystem::path(path).filename().string();
                const size_t cut = stem.find(".bins.tsv");
                if (cut != std::string::npos) stem.resize(cut);
                bool used = false;
                for (size_t fi = 0; fi < all_filters.size(); ++fi)
                    if (all_filters[fi]->name == stem) { bin_records[fi] = read_bin_map(path); used = true; }
                if (!used) throw std::runtime_error("--bin-map " + path + ": no filter named " + stem);
            }
        }
        if (opt.report_bins) {
            bins_out.open(std::filesystem::path(config.output_dir) / "classified_bins.tsv");
            if (!bins_out) { std::cerr << "ERROR: Unable to open the file: classified_bins.tsv" << std::endl; return; }
            bins_out << "read_id\tfilter\tbest_bin\tstrand\tmax_count\tthreshold\thit_bins\tchunk" << (opt.bin_maps.empty() ? "" : "\trecord_id") << '\n';
        }
        if (opt.report_spans) {
            spans_out.open(std::filesystem::path(config.output_dir) / "classified_spans.tsv");
            if (!spans_out) { std::cerr << "ERROR: Unable to open the file: classified_spans.tsv" << std::endl; return; }
            spans_out << "read_id\tfilter\tbin" << (opt.bin_maps.empty() ? "" : "\trecord_id")
                      << "\tstrand\tn_kmers\tcount\tfirst\tlast\trun_start\trun_len\tcovered\n";
        }
        if (opt.report_prefixes) {
            prefixes_out.open(std::filesystem::path(config.output_dir) / "classified_prefixes.tsv");
            if (!prefixes_out) { std::cerr << "ERROR: Unable to open the file: classified_prefixes.tsv" << std::endl; return; }
            prefixes_out << "read_id\tlength";
            for (uint32_t c : opt.prefix_lens) {
                prefixes_out << "\tprefix_len@" << c << "\tdecision@" << c << "\tbest_target@" << c;
                for (const interleave::IBFMeta* f : all_filters) prefixes_out << "\tmax_" << f->name << '@' << c;
            }
            prefixes_out << '\n';
        }
        if (opt.report_hits) {
            hits_out.open(std::filesystem::path(config.output_dir) / "classified_hits.tsv");
            if (!hits_out) { std::cerr << "ERROR: Unable to open the file: classified_hits.tsv" << std::endl; return; }
            hits_out << "read_id\tfilter\tbin" << (opt.bin_maps.empty() ? "" : "\trecord_id") << "\tstrand\tcount\tthreshold\tn_hits\n";
            size_t total_bins = 0;
            for (const interleave::IBFMeta* f : all_filters) total_bins += (size_t)f->filter.noOfBins;
            bin_profile.assign(total_bins, 0);
        }
        seqio::MappedFile mapped(read_file.string());
        if (!mapped.is_open()) {
            std::cerr << "ERROR: Unable to open the file: " << read_file.string() << std::endl;
            return;
        }
        std::cout << '\n' << "Classification results of: " << read_file.string() << '\n' << '\n';

        const uint32_t chunk_length = (uint32_t)config.IBF_Parsed.chunk_length;
        const uint32_t max_chunks = (uint8_t)config.IBF_Parsed.max_chunks;  // "uint8_t i" in the reference

        // pass 1 over a classified segment: which file every read goes to and how many bytes it takes there (classify.hpp:289-316)
        auto fasta_bytes = [&](const seqio::Record& r, bool one_line) -> uint64_t {
            // target FASTAs: `targetFastas[i] << ">" << id << endl << seq << endl` -- the raw read on one line;
            // unclassified.fasta: seqan::writeRecord(..., (seqan::Dna5String)seq) -- SeqAn's default 70-column lines
            return 1 + (uint64_t)r.id_len + 1 + r.seq_len + (one_line ? 1 : (r.seq_len + 69) / 70);
        };
        auto size_segment = [&](const seqio::Segment& seg, const std::vector<ReadState>& state) {
            SegmentOutput so;
            so.bytes.assign(n_out, 0);
            so.per_target.assign(TargetFilters.size(), 0);
            const std::vector<seqio::Record>& recs = seg.batch.records;
            for (size_t i = 0; i < recs.size(); ++i) {
                const seqio::Record& r = recs[i];
                if (r.seq_len < chunk_length) continue;
                if (state[i].failed) {  // classify.hpp:306-316
                    so.failed++;
                    so.error_lines.push_back("Error classifying Read : " + std::string(r.id, r.id_len) + "(Len=" + std::to_string(r.seq_len) + ")");
                    continue;
                }
                if (state[i].classified) {
                    so.found++;
                    if (!(target && state[i].best >= 0)) continue;
                    so.per_target[state[i].best] += 1;
                    so.bytes[state[i].best] += fasta_bytes(r, true);
                } else {
                    so.bytes[n_out - 1] += fasta_bytes(r, false);
                }
            }
            return so;
        };
        // pass 2: the FASTA text of the segment, written where pass 1 and the reservation said (out[f] = cursor over this segment's share of file f)
        auto format_segment = [&](const seqio::Segment& seg, const std::vector<ReadState>& state, std::vector<seqio::OrderedOutput::Writer>& out) {
            const std::vector<seqio::Record>& recs = seg.batch.records;
            for (size_t i = 0; i < recs.size(); ++i) {
                const seqio::Record& r = recs[i];
                if (r.seq_len < chunk_length || state[i].failed) continue;
                size_t f = n_out - 1;  // unclassified.fasta
                if (state[i].classified) {
                    if (!(target && state[i].best >= 0)) continue;
                    f = (size_t)state[i].best;
                }
                const bool one_line = f != n_out - 1;
                char* dst = out[f].take((size_t)fasta_bytes(r, one_line));
                *dst++ = '>';
                std::memcpy(dst, r.id, r.id_len);
                dst += r.id_len;
                *dst++ = '\n';
                if (one_line) {
                    std::memcpy(dst, r.seq, r.seq_len);
                    dst[r.seq_len] = '\n';
                } else {
                    // the Dna5 alphabet (upper case, everything but ACGT[U] becomes N) in 70-column lines
                    for (size_t p = 0; p < r.seq_len; p += 70) {
                        const size_t n = std::min<size_t>(70, r.seq_len - p);
                        dna5_map(dst, r.seq + p, n);
                        dst[n] = '\n';
                        dst += n + 1;
                    }
                }
            }
        };

        // first chunks are staged in page-locked memory: the copy to the GPU is then a plain DMA (a pageable source is
        // pinned on the fly by the runtime, under the same mm lock the parser threads' page faults need)
        seqio::BlockAllocator pinned;
        pinned.alloc = [](size_t bytes) -> void* { void* p = nullptr; return rb_host_alloc(bytes, &p) == RB_OK ? p : nullptr; };
        pinned.release = [](void* p) { rb_host_free(p); };
        seqio::ParallelReader reader(mapped.data(), mapped.size(), opt.threads, opt.bytes(), chunk_length, pinned);
        double wait_reader_s = 0.0, wait_turn_s = 0.0, format_s = 0.0;
        auto seconds_since = [](std::chrono::steady_clock::time_point t) {
            return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
        };
        // the chunk loop of one segment (classify.hpp:262-299, batch-wise): the reads go to the GPU in calls of at most
        // batch_reads; chunk 0 comes ready-made from the parser threads, later chunks are gathered here for the reads that
        // are still unclassified
        auto classify_segment = [&](const seqio::Segment& seg, std::vector<ReadState>& state, std::vector<uint64_t>& seg_profile,
                                    std::vector<uint64_t>& seg_tally) {
            const std::vector<seqio::Record>& recs = seg.batch.records;
            std::vector<char> flat;
            std::vector<uint64_t> offs;
            std::vector<uint32_t> lens;
            std::vector<size_t> idx;
            if (opt.report_prefixes) {
                // every read of the segment, whole, in the run's mode: one rb_prefix_batch per batch_reads reads
                const size_t nf = all_filters.size(), P = n_cp;
                for (size_t b0 = 0; b0 < recs.size(); b0 += opt.batch_reads) {
                    const size_t nb = std::min(recs.size(), b0 + opt.batch_reads) - b0;
                    flat.clear();
                    offs.clear();
                    lens.clear();
                    for (size_t j = 0; j < nb; ++j) {
                        const seqio::Record& r = recs[b0 + j];
                        offs.push_back(flat.size());
                        lens.push_back((uint32_t)r.seq_len);
                        flat.insert(flat.end(), r.seq, r.seq + r.seq_len);
                    }
                    if (flat.empty()) flat.push_back('N');
                    std::vector<uint16_t> mc(nb * P * nf);
                    std::vector<uint8_t> dec(nb * P), ps(nb * P);
                    std::vector<int32_t> bt(nb * P);
                    std::vector<uint32_t> pl(nb * P), fd(nb);
                    rb_prefix_out po{mc.data(), dec.data(), bt.data(), ps.data(), pl.data(), fd.data()};
                    interleave::throw_status(rb_prefix_batch(interleave::detail::engine_for(DepletionFilters, TargetFilters), flat.data(), offs.data(),
                                                             lens.data(), nb, nullptr, 0, opt.prefix_lens.data(), (uint32_t)P, Conf.error_rate,
                                                             Conf.significance, RB_MODE_CLASSIFY_CHUNK, &po),
                                             "rb_prefix_batch");
                    for (size_t j = 0; j < nb; ++j) {
                        const seqio::Record& r = recs[b0 + j];
                        size_t w = 0;
                        while (w < r.id_len && r.id[w] != ' ' && r.id[w] != '\t') ++w;
                        std::string& row = state[b0 + j].prefix_row;
                        row.append(r.id, w);
                        row += '\t' + std::to_string(r.seq_len);
                        for (size_t p = 0; p < P; ++p) {
                            const size_t q = j * P + p;
                            row += '\t' + std::to_string(pl[q]) + '\t' + std::to_string(dec[q]) + '\t' + std::to_string(bt[q]);
                            for (size_t fi = 0; fi < nf; ++fi) row += '\t' + std::to_string(mc[q * nf + fi]);
                            uint64_t* t = seg_tally.data() + p * kPrefixTallies;
                            if (r.seq_len >= opt.prefix_lens[p]) t[0] += 1;
                            t[1 + std::min<unsigned>(dec[q], 2u)] += 1;
                            if (fd[j] == p) t[4] += 1;
                            if (p > 0 && dec[q] != dec[q - 1]) t[5] += 1;
                        }
                        row += '\n';
                    }
                }
                flat.clear();
            }
            for (size_t b0 = 0; b0 < seg.prefix_idx.size(); b0 += opt.batch_reads) {
                const size_t b1 = std::min(seg.prefix_idx.size(), b0 + opt.batch_reads);
                std::vector<size_t> active(b1 - b0);
                for (size_t j = b0; j < b1; ++j) active[j - b0] = seg.prefix_idx[j];
                for (uint32_t c = 0; c < max_chunks && !active.empty(); ++c) {
                    const char* base = nullptr;
                    offs.clear();
                    lens.clear();
                    idx.clear();
                    if (c == 0) {
                        base = seg.prefix + b0 * (size_t)chunk_length;
                        for (size_t j = 0; j < active.size(); ++j) {
                            offs.push_back(j * (uint64_t)chunk_length);
                            lens.push_back(chunk_length);
                        }
                        idx = active;
                    } else {
                        flat.clear();
                        for (size_t i : active) {
                            const seqio::Record& r = recs[i];
                            uint64_t fragend = (uint64_t)(c + 1) * chunk_length, fragstart = (uint64_t)c * chunk_length;
                            if (fragend > r.seq_len) fragend = r.seq_len;
                            if (fragstart > fragend) { state[i].failed = true; continue; }  // undefined infix in the reference
                            offs.push_back(flat.size());
                            lens.push_back((uint32_t)(fragend - fragstart));
                            flat.insert(flat.end(), r.seq + fragstart, r.seq + fragend);
                            idx.push_back(i);
                        }
                        if (flat.empty()) flat.push_back('N');
                        base = flat.data();
                    }
                    std::vector<size_t> next;
                    if (!idx.empty()) {
                        interleave::BatchResult res =
                            multi ? multi->classify_flat(Conf, base, offs.data(), lens.data(), idx.size(), RB_MODE_CLASSIFY_CHUNK)
                                  : interleave::classify_batch_flat(DepletionFilters, TargetFilters, Conf, base, offs.data(),
                                                                    lens.data(), idx.size(), RB_MODE_CLASSIFY_CHUNK);
                        std::vector<uint32_t> located;  // --report-bins: the work items this chunk classified
                        for (size_t j = 0; j < idx.size(); ++j) {
                            ReadState& st = state[idx[j]];
                            if (res.status[j] != RB_OK) { st.failed = true; continue; }  // exception -> failed++ (:306-316)
                            if (res.decision[j]) {
                                st.classified = true;
                                st.best = target ? res.best_target[j] : -1;
                                if (opt.report_bins || opt.report_hits || opt.report_spans) located.push_back((uint32_t)j);
                            } else {
                                next.push_back(idx[j]);
                            }
                        }
                        if (opt.report_hits && !located.empty()) {
                            // every (bin, strand) at or above the decision threshold of the reads this chunk classified; the profile of
                            // the segment is added to the run's when the segment's turn to write comes
                            // the record buffer of a call stays at or below 64 MiB whatever --max-hits is: the reads go in pieces
                            const size_t nf = all_filters.size(), cap = opt.max_hits;
                            const size_t piece = std::max<size_t>(1, ((size_t)64 << 20) / (nf * cap * sizeof(rb_hit)));
                            for (size_t p0 = 0; p0 < located.size(); p0 += piece) {
                            const size_t nl = std::min(piece, located.size() - p0);
                            std::vector<rb_hit> hv(nl * nf * cap);
                            std::vector<uint32_t> nh(nl * nf);
                            std::vector<uint8_t> hs(nl);
                            rb_hits_out ho{hv.data(), nh.data(), hs.data(), seg_profile.data()};
                            interleave::throw_status(rb_hits_batch(interleave::detail::engine_for(DepletionFilters, TargetFilters), base, offs.data(),
                                                                   lens.data(), idx.size(), located.data() + p0, nl, Conf.error_rate, Conf.significance, 0,
                                                                   opt.max_hits, &ho),
                                                     "rb_hits_batch");
                            for (size_t q = 0; q < nl; ++q) {
                                if (hs[q] != RB_OK) continue;
                                const size_t j = located[p0 + q];
                                const seqio::Record& r = recs[idx[j]];
                                size_t w = 0;
                                while (w < r.id_len && r.id[w] != ' ' && r.id[w] != '\t') ++w;
                                std::string& rows = state[idx[j]].hit_rows;
                                for (size_t fi = 0; fi < nf; ++fi) {
                                    const uint16_t t = rb_threshold(lens[j], all_filters[fi]->filter.kmerSize, Conf.error_rate, Conf.significance);
                                    const uint32_t total = nh[q * nf + fi];
                                    const size_t kept = std::min<size_t>(total, cap);
                                    for (size_t h = 0; h < kept; ++h) {
                                        const rb_hit& rec = hv[(q * nf + fi) * cap + h];
                                        rows.append(r.id, w);
                                        rows += '\t' + all_filters[fi]->name + '\t' + std::to_string(rec.bin);
                                        if (!opt.bin_maps.empty()) {
                                            const std::vector<std::string>& map = bin_records[fi];
                                            rows += '\t' + ((rec.bin < map.size() && !map[rec.bin].empty()) ? map[rec.bin] : std::string("-"));
                                        }
                                        rows += std::string("\t") + (rec.strand ? '-' : '+') + '\t' + std::to_string(rec.count) + '\t' + std::to_string(t) + '\t' +
                                                std::to_string(total) + '\n';
                                    }
                                }
                            }
                            }
                        }
                        if ((opt.report_bins || opt.report_spans) && !located.empty()) {
                            const size_t nf = all_filters.size(), nl = located.size();
                            std::vector<uint16_t> mc(nl * nf);
                            std::vector<int32_t> bb(nl * nf);
                            std::vector<uint8_t> bs(nl * nf), ls(nl);
                            std::vector<uint32_t> hb(nl * nf);
                            rb_locate_out lo{mc.data(), bb.data(), bs.data(), hb.data(), ls.data()};
                            interleave::throw_status(rb_locate_batch(interleave::detail::engine_for(DepletionFilters, TargetFilters), base, offs.data(),
                                                                     lens.data(), idx.size(), located.data(), nl, Conf.error_rate, Conf.significance, &lo),
                                                     "rb_locate_batch");
                            for (size_t q = 0; q < nl; ++q) {
                                if (ls[q] != RB_OK) continue;
                                const size_t j = located[q];
                                const seqio::Record& r = recs[idx[j]];
                                size_t w = 0;
                                while (w < r.id_len && r.id[w] != ' ' && r.id[w] != '\t') ++w;
                                std::string& rows = state[idx[j]].bin_rows;
                                for (size_t fi = 0; fi < nf; ++fi) {
                                    // a line per filter that matched the chunk: max_matches' predicate, count >= threshold (and a count at all)
                                    const uint16_t t = rb_threshold(lens[j], all_filters[fi]->filter.kmerSize, Conf.error_rate, Conf.significance);
                                    const uint16_t m = mc[q * nf + fi];
                                    if (m == 0 || m < t) { bb[q * nf + fi] = -1; continue; }  // (-1: the spans report below asks nothing of this filter)
                                    if (!opt.report_bins) continue;
                                    rows.append(r.id, w);
                                    rows += '\t' + all_filters[fi]->name + '\t' + std::to_string(bb[q * nf + fi]) + '\t' + (bs[q * nf + fi] ? '-' : '+') + '\t' +
                                            std::to_string(m) + '\t' + std::to_string(t) + '\t' + std::to_string(hb[q * nf + fi]) + '\t' + std::to_string(c);
                                    if (!opt.bin_maps.empty()) {
                                        const std::vector<std::string>& map = bin_records[fi];
                                        const int32_t b = bb[q * nf + fi];
                                        rows += '\t' + ((b >= 0 && (size_t)b < map.size() && !map[b].empty()) ? map[b] : std::string("-"));
                                    }
                                    rows += '\n';
                                }
                            }
                            if (opt.report_spans) {
                                // per filter that matched: the located best bin of every such read, one query each; the record of the best strand
                                std::vector<rb_span_query> qs;
                                std::vector<rb_span> sp;
                                std::vector<uint32_t> nk;
                                std::vector<uint8_t> ss;
                                for (size_t fi = 0; fi < nf; ++fi) {
                                    qs.clear();
                                    for (size_t q = 0; q < nl; ++q)
                                        if (ls[q] == RB_OK && bb[q * nf + fi] >= 0) qs.push_back(rb_span_query{(uint32_t)q, (uint32_t)bb[q * nf + fi]});
                                    if (qs.empty()) continue;
                                    sp.resize(qs.size() * 2);
                                    nk.resize(qs.size());
                                    ss.resize(qs.size());
                                    rb_spans_out so{sp.data(), nullptr, nk.data(), ss.data()};
                                    interleave::throw_status(rb_spans_batch(interleave::detail::engine_for(DepletionFilters, TargetFilters), base, offs.data(),
                                                                            lens.data(), idx.size(), located.data(), nl, fi, qs.data(), qs.size(), 0, &so),
                                                             "rb_spans_batch");
                                    const uint32_t at = c * chunk_length;  // positions in the read's coordinates
                                    for (size_t x = 0; x < qs.size(); ++x) {
                                        if (ss[x] != RB_OK) continue;
                                        const size_t q = qs[x].item, j = located[q];
                                        const seqio::Record& r = recs[idx[j]];
                                        size_t w = 0;
                                        while (w < r.id_len && r.id[w] != ' ' && r.id[w] != '\t') ++w;
                                        const uint8_t strand = bs[q * nf + fi];
                                        const rb_span& rec = sp[2 * x + strand];
                                        std::string& rows = state[idx[j]].span_rows;
                                        rows.append(r.id, w);
                                        rows += '\t' + all_filters[fi]->name + '\t' + std::to_string(qs[x].bin);
                                        if (!opt.bin_maps.empty()) {
                                            const std::vector<std::string>& map = bin_records[fi];
                                            rows += '\t' + ((qs[x].bin < map.size() && !map[qs[x].bin].empty()) ? map[qs[x].bin] : std::string("-"));
                                        }
                                        rows += std::string("\t") + (strand ? '-' : '+') + '\t' + std::to_string(nk[x]) + '\t' + std::to_string(rec.count) + '\t' +
                                                std::to_string(rec.first + at) + '\t' + std::to_string(rec.last + at) + '\t' + std::to_string(rec.run_start + at) + '\t' +
                                                std::to_string(rec.run_len) + '\t' + std::to_string(rec.covered) + '\n';
                                    }
                                }
                            }
                        }
                    }
                    active.swap(next);
                }
            }
        };
        // classifier threads: each takes the next segment in file order, runs its chunk loop on an engine of its own (the
        // mirror keeps one engine per calling thread) and hands the result to the writer when its turn has come -- while
        // one thread waits for the GPU, the other prepares and post-processes its segment
        std::mutex rmu, omu;
        std::condition_variable ocv;
        uint64_t next_seq = 0, write_seq = 0;
        std::string worker_error;
        std::mutex cal_mu;
        std::condition_variable cal_cv;
        unsigned cal_parties = 0, cal_arrived = 0;  // (cal_parties is set before the first classifier starts)
        auto classifier = [&] {
            try {
                if ((opt.report_bins || opt.report_hits) && !multi && opt.pass_lists != RB_PASS_LISTS_OFF)
                    interleave::throw_status(rb_engine_set_pass_lists(interleave::detail::engine_for(DepletionFilters, TargetFilters), opt.pass_lists),
                                             "rb_engine_set_pass_lists");
                if (!multi && opt.wide_lists != RB_PASS_LISTS_OFF)
                    interleave::throw_status(rb_engine_set_wide_lists(interleave::detail::engine_for(DepletionFilters, TargetFilters), opt.wide_lists),
                                             "rb_engine_set_wide_lists");
                if ((opt.report_bins || opt.report_hits) && !multi && opt.wide_pass_lists != RB_PASS_LISTS_OFF)
                    interleave::throw_status(rb_engine_set_wide_pass_lists(interleave::detail::engine_for(DepletionFilters, TargetFilters), opt.wide_pass_lists),
                                             "rb_engine_set_wide_pass_lists");
                if (opt.report_prefixes && !multi && opt.prefix_lists != RB_PASS_LISTS_OFF)
                    interleave::throw_status(rb_engine_set_prefix_lists(interleave::detail::engine_for(DepletionFilters, TargetFilters), opt.prefix_lists),
                                             "rb_engine_set_prefix_lists");
                if (opt.report_prefixes && !multi && opt.wide_prefix_lists != RB_PASS_LISTS_OFF)
                    interleave::throw_status(rb_engine_set_wide_prefix_lists(interleave::detail::engine_for(DepletionFilters, TargetFilters), opt.wide_prefix_lists),
                                             "rb_engine_set_wide_prefix_lists");
                if (opt.calibrate && !multi) {
                    // one engine at a time, and nobody classifies before the last engine is calibrated: an engine timed beside
                    // another thread's classification picks its windows from noise
                    std::unique_lock<std::mutex> lock(cal_mu);
                    uint32_t n_tables = 0, n_changed = 0;
                    int rc = RB_ERR_INVALID_ARG;
                    try {
                        rc = rb_engine_calibrate(interleave::detail::engine_for(DepletionFilters, TargetFilters), opt.batch_reads, chunk_length, 40.0,
                                                 &n_tables, &n_changed);
                    } catch (...) {
                        ++cal_arrived;  // (the others must not wait for a thread that is on its way out)
                        cal_cv.notify_all();
                        throw;
                    }
                    if (rc != RB_OK) log_line("warn", std::string("calibration skipped: ") + rb_last_error());
                    else log_line("info", "calibrated " + std::to_string(n_tables) + " phased table(s), " + std::to_string(n_changed) + " window(s) changed");
                    ++cal_arrived;
                    cal_cv.notify_all();
                    cal_cv.wait(lock, [&] { return cal_arrived >= cal_parties; });
                }
                for (;;) {
                    std::unique_ptr<seqio::Segment> seg;
                    uint64_t seq = 0;
                    {
                        std::lock_guard<std::mutex> lock(rmu);
                        const auto tr = std::chrono::steady_clock::now();
                        seg = reader.next();
                        wait_reader_s += seconds_since(tr);
                        if (!seg) return;
                        seq = next_seq++;
                        readCounter += seg->batch.records.size();
                        too_short += seg->batch.records.size() - seg->prefix_idx.size();  // classify.hpp:247-250
                        classify_reads_n += seg->prefix_idx.size();
                        if (!seg->batch.error.empty()) std::cerr << "ERROR: " << seg->batch.error << std::endl;
                    }
                    std::vector<ReadState> state(seg->batch.records.size());
                    const auto t0 = std::chrono::steady_clock::now();
                    std::vector<uint64_t> seg_profile(bin_profile.size(), 0), seg_tally(prefix_tally.size(), 0);
                    classify_segment(*seg, state, seg_profile, seg_tally);
                    const double secs = seconds_since(t0);
                    SegmentOutput so = size_segment(*seg, state);
                    std::vector<uint64_t> at(n_out, 0);
                    {
                        // this segment's turn: its share of every output file starts where the segment before it ends
                        const auto tw = std::chrono::steady_clock::now();
                        std::unique_lock<std::mutex> lock(omu);
                        ocv.wait(lock, [&] { return write_seq == seq || write_seq == ~0ULL; });
                        if (write_seq == ~0ULL) return;  // another worker failed
                        wait_turn_s += seconds_since(tw);
                        classify_seconds += secs;
                        for (size_t f = 0; f < n_out; ++f)
                            if (outputs[f]->is_open()) at[f] = outputs[f]->reserve(so.bytes[f]);
                        found += so.found;
                        failed += (uint16_t)so.failed;
                        for (const std::string& l : so.error_lines) log_line("error", l);
                        if (opt.report_bins)
                            for (const ReadState& rs : state) bins_out << rs.bin_rows;
                        if (opt.report_spans)
                            for (const ReadState& rs : state) spans_out << rs.span_rows;
                        if (opt.report_prefixes) {
                            for (const ReadState& rs : state) prefixes_out << rs.prefix_row;
                            for (size_t b = 0; b < prefix_tally.size(); ++b) prefix_tally[b] += seg_tally[b];
                        }
                        if (opt.report_hits) {
                            for (const ReadState& rs : state) hits_out << rs.hit_rows;
                            for (size_t b = 0; b < bin_profile.size(); ++b) bin_profile[b] += seg_profile[b];
                        }
                        for (size_t f = 0; f < TargetFilters.size(); ++f) TargetFilters[f].classified += so.per_target[f];
                        ++write_seq;
                    }
                    ocv.notify_all();
                    // ... and the text itself, by every classifier thread at once
                    const auto tf = std::chrono::steady_clock::now();
                    std::vector<seqio::OrderedOutput::Writer> out(n_out);
                    // (a file that could not be opened -- target FASTAs are not checked by the reference -- is formatted into the void)
                    for (size_t f = 0; f < n_out; ++f) out[f] = outputs[f]->writer(at[f], so.bytes[f]);
                    format_segment(*seg, state, out);
                    for (size_t f = 0; f < n_out; ++f) {
                        const bool complete = outputs[f]->is_open() ? out[f].finish() : true;
                        if (!complete) throw std::runtime_error("output layout mismatch");
                    }
                    out.clear();            // (the cursors first: their buffers are on their way to the files' writer threads)
                    const size_t seg_index = seg->index;
                    seg.reset();
                    reader.release(seg_index);  // the records of this segment are not looked at again
                    {
                        std::lock_guard<std::mutex> lock(omu);
                        format_s += seconds_since(tf);
                    }
                }
            } catch (const std::exception& ex) {
                std::lock_guard<std::mutex> lock(omu);
                if (worker_error.empty()) worker_error = ex.what();
                write_seq = ~0ULL;  // nobody's turn any more: the other workers stop at their hand-over
                ocv.notify_all();
            }
        };
        unsigned n_classifiers = opt.classify_threads ? opt.classify_threads
                                                      : (config.IBF_Parsed.threads > 1 ? (unsigned)config.IBF_Parsed.threads : 4u);
        {
            // (a multi-device pool spreads every call over its devices itself; two callers keep it fed while one formats)
            if (multi) n_classifiers = std::min(n_classifiers, 2u);
            cal_parties = n_classifiers;
            std::vector<std::thread> workers;
            for (unsigned i = 1; i < n_classifiers; ++i) workers.emplace_back(classifier);
            classifier();
            for (std::thread& t : workers) t.join();
        }
        if (!worker_error.empty()) throw std::runtime_error(worker_error);
        for (auto& o : outputs) {
            o->close();
            if (!o->ok()) std::cerr << "ERROR: writing an output file failed: " << o->error() << std::endl;
        }
        if (opt.report_prefixes) {
            std::ofstream sum(std::filesystem::path(config.output_dir) / "prefix_summary.tsv");
            if (!sum) std::cerr << "ERROR: Unable to open the file: prefix_summary.tsv" << std::endl;
            else sum << "prefix_len\treads_reaching\tdecision_0\tdecision_1\tdecision_2\tfirst_decided\tchanged\n";
            for (size_t p = 0; sum && p < n_cp; ++p) {
                sum << opt.prefix_lens[p];
                for (size_t t = 0; t < kPrefixTallies; ++t) sum << '\t' << prefix_tally[p * kPrefixTallies + t];
                sum << '\n';
            }
        }
        if (opt.report_hits) {
            std::ofstream prof(std::filesystem::path(config.output_dir) / "bin_profile.tsv");
            if (!prof) std::cerr << "ERROR: Unable to open the file: bin_profile.tsv" << std::endl;
            else prof << "filter\tbin\trecord_id\treads\n";
            size_t at = 0;
            for (size_t fi = 0; prof && fi < all_filters.size(); ++fi) {
                const size_t nb = (size_t)all_filters[fi]->filter.noOfBins;
                for (size_t b = 0; b < nb; ++b)
                    if (bin_profile[at + b])
                        prof << all_filters[fi]->name << '\t' << b << '\t'
                             << ((b < bin_records[fi].size() && !bin_records[fi][b].empty()) ? bin_records[fi][b] : std::string("-")) << '\t'
                             << bin_profile[at + b] << '\n';
                at += nb;
            }
        }
        const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
        const double avg = classify_reads_n ? classify_seconds / (double)classify_reads_n : 0.0;
        std::cout << "------------------------------- Final Results -------------------------------" << std::endl;
        std::cout << "Number of classified reads                         :   " << found << std::endl;
        std::cout << "Number of of too short reads (len < " << config.IBF_Parsed.chunk_length << ")           :   " << too_short << std::endl;
        std::cout << "Number of all reads                                :   " << readCounter << std::endl;
        for (interleave::IBFMeta& f : TargetFilters)
            std::cout << f.name << "\t : " << f.classified << "\t\t" << ((float)f.classified) / ((float)readCounter) << std::endl;
        std::cout << "Average Processing Time Read Classification        :   " << avg << std::endl;
        std::cout << "-----------------------------------------------------------------------------------" << std::endl;
        log_line("info", "classified " + std::to_string(found) + " too_short " + std::to_string(too_short) + " failed " +
                             std::to_string(failed) + " all " + std::to_string(readCounter) + " reads of " + read_file.string());
        std::cout << "RESULT found=" << found << " failed=" << failed << " too_short=" << too_short
                  << " readCounter=" << readCounter << std::endl;
        std::cout << "THROUGHPUT reads_per_s=" << (wall > 0 ? (double)readCounter / wall : 0.0) << " wall_s=" << wall
                  << " classify_s=" << classify_seconds << " wait_reader_s=" << wait_reader_s
                  << " wait_turn_s=" << wait_turn_s << " format_s=" << format_s << " classifiers=" << n_classifiers
                  << " parsers=" << opt.threads << std::endl;
        ClassificationResults_.found = found;
        ClassificationResults_.failed = failed;
        ClassificationResults_.too_short = too_short;
        ClassificationResults_.readCounter = readCounter;
        for (interleave::IBFMeta& f : TargetFilters) f.classified = 0;
    }
}

// usage = "target" as an OFFLINE REPLAY of the live classification step (src/main/adaptive_sampling.hpp:214-356: what
// happens to a basecalled chunk between classification_queue and action_queue).  The MinKNOW gRPC client and the
// basecallers are out of scope; what they would deliver -- basecalled chunks, in arrival order -- comes from
// [IBF] read_files instead: one record per chunk, the first word of the record id is the read id (chunks of one read
// carry the same id and appear in the order they were sequenced; anything after the first blank, e.g. "ch=12 chunk=3",
// is carried along as a comment).  The chunks go through rb_live_process in micro-batches of `live_batch` records (what
// the basecaller threads would have queued while the GPU was busy), with the reference's bookkeeping: once_seen,
// concatenation of undecided chunks, the 1500 bp cut-off, decision -> action (Data::sendActions, Data.cpp:169-187).
// Output: <output_directory>/live_actions.tsv, one line per chunk in arrival order:
//   record  read_id  action(none|unblock_read|stop_receiving_data)  status  classified_length
// and the tallies the reference logs for a run.
static int replay_target(ConfigReader& config, std::vector<interleave::IBFMeta>& DepletionFilters,
                         std::vector<interleave::IBFMeta>& TargetFilters, size_t live_batch)
{
    rb_engine* engine = interleave::detail::engine_for(DepletionFilters, TargetFilters);
    rb_live* live = nullptr;
    // Conf.significance = 0.95, Conf.error_rate = exp_seq_error_rate (adaptive_sampling.hpp:563-566); 1500 bp cut-off (:315)
    interleave::throw_status(rb_live_create(engine, config.IBF_Parsed.error_rate, 0.95, 1500, &live), "rb_live_create");
    std::ofstream out(std::filesystem::path(config.output_dir) / "live_actions.tsv");
    out << "record\tread_id\taction\tstatus\tclassified_length\n";
    static const char* kAction[3] = {"none", "unblock_read", "stop_receiving_data"};
    uint64_t n_records = 0, n_unblock = 0, n_stop = 0, n_failed = 0, n_calls = 0;
    double classify_s = 0.0;
    const auto t_begin = std::chrono::steady_clock::now();
    for (const std::filesystem::path& read_file : config.IBF_Parsed.read_files) {
        seqio::MappedFile mapped(read_file.string());
        if (!mapped.is_open()) { rb_live_destroy(live); throw interleave::FileParserException("ERROR: Unable to open the file: " + read_file.string()); }
        seqio::Parser parser(mapped.data(), mapped.size());
        seqio::Batch batch;
        for (;;) {
            parser.next_batch(batch, live_batch);
            const size_t n = batch.records.size();
            if (n) {
                std::string ids, seqs;
                std::vector<uint64_t> id_off(n), off(n);
                std::vector<uint32_t> id_len(n), len(n);
                for (size_t i = 0; i < n; ++i) {
                    const seqio::Record& r = batch.records[i];
                    size_t w = 0;
                    while (w < r.id_len && r.id[w] != ' ' && r.id[w] != '\t') ++w;
                    id_off[i] = ids.size(); id_len[i] = (uint32_t)w; ids.append(r.id, w);
                    off[i] = seqs.size(); len[i] = (uint32_t)r.seq_len; seqs.append(r.seq, r.seq_len);
                }
                if (seqs.empty()) seqs.push_back('N');
                std::vector<uint8_t> action(n), status(n);
                std::vector<uint32_t> clen(n);
                const auto t0 = std::chrono::steady_clock::now();
                const int rc = rb_live_process(live, ids.data(), id_off.data(), id_len.data(), seqs.data(), off.data(), len.data(), n,
                                               action.data(), status.data(), clen.data());
                classify_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (rc != RB_OK) { rb_live_destroy(live); interleave::throw_status(rc, "rb_live_process"); }
                ++n_calls;
                for (size_t i = 0; i < n; ++i) {
                    out << n_records + i << '\t';
                    out.write(ids.data() + id_off[i], id_len[i]);
                    out << '\t' << kAction[action[i] < 3 ? action[i] : 0] << '\t' << (int)status[i] << '\t' << clen[i] << '\n';
                    n_unblock += action[i] == 1;
                    n_stop += action[i] == 2;
                    if (status[i] != RB_OK) {
                        ++n_failed;  // adaptive_sampling.hpp:340-349: logged, no action, state untouched
                        log_line("error", "Error classifying Read : " + std::string(ids.data() + id_off[i], id_len[i]) + "(Len=" + std::to_string(len[i]) + ")");
                    }
                }
                n_records += n;
            }
            if (!batch.error.empty()) { rb_live_destroy(live); throw interleave::FileParserException("ERROR: " + batch.error); }
            if (batch.eof) break;
        }
    }
    const size_t pending = rb_live_pending(live);
    rb_live_destroy(live);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    std::cout << "------------------------------- Live Replay Results -------------------------------" << std::endl;
    std::cout << "Number of chunks replayed                          :   " << n_records << std::endl;
    std::cout << "Number of unblock_read actions                     :   " << n_unblock << std::endl;
    std::cout << "Number of stop_receiving_data actions              :   " << n_stop << std::endl;
    std::cout << "Number of chunks that failed to classify           :   " << n_failed << std::endl;
    std::cout << "Reads still waiting for more data (once_seen)      :   " << pending << std::endl;
    std::cout << "LIVE chunks=" << n_records << " unblock=" << n_unblock << " stop=" << n_stop << " failed=" << n_failed
              << " pending=" << pending << " calls=" << n_calls << " classify_s=" << classify_s << " wall_s=" << wall << std::endl;
    log_line("info", "live replay: " + std::to_string(n_records) + " chunks, " + std::to_string(n_unblock) + " unblock, " +
                         std::to_string(n_stop) + " stop_receiving");
    return 0;
}

static int run_program(ConfigReader& config, const IngestOptions& opt, const std::vector<int>& devices)
{
    config.parse();
    config.createLog(config.usage);  // main.cpp:283
    g_log.open(config.log_dir / "ReadBouncerLog.txt", std::ios::app);
    log_line("info", "usage " + config.usage);
    if (config.usage == "build") {  // main.cpp:286-344
        for (const auto& files : {config.IBF_Parsed.target_files, config.IBF_Parsed.deplete_files}) {
            for (std::filesystem::path file : files) {
                std::filesystem::path out = config.output_dir;
                out /= file.filename();
                out.replace_extension("ibf");
                buildIBF(config, file.string(), out.string());
            }
        }
        return 0;
    }
    if (config.usage == "classify") {  // main.cpp:346-376
        const auto t_load = std::chrono::steady_clock::now();
        std::vector<interleave::IBFMeta> DepletionFilters = getIBF(config, true, false);
        std::vector<interleave::IBFMeta> TargetFilters = getIBF(config, false, true);
        const double load_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_load).count();
        const auto t_cls = std::chrono::steady_clock::now();
        classify_reads(config, DepletionFilters, TargetFilters, opt, devices);
        std::cout << "PHASES load_filters_s=" << load_s << " classify_reads_s="
                  << std::chrono::duration<double>(std::chrono::steady_clock::now() - t_cls).count() << std::endl;
        return 0;
    }
    if (config.usage == "target") {  // main.cpp:365-378, with the chunk source replaced (see replay_target)
        if (config.IBF_Parsed.read_files.empty()) {  // before any filter is loaded or built
            std::cerr << "usage \"target\": the live MinKNOW/basecaller connection is outside this engine's scope; list pre-basecalled "
                         "chunk files under [IBF] read_files to replay them through the live classification step" << std::endl;
            return 2;
        }
        std::vector<interleave::IBFMeta> DepletionFilters = getIBF(config, true, false);
        std::vector<interleave::IBFMeta> TargetFilters = getIBF(config, false, true);
        return replay_target(config, DepletionFilters, TargetFilters, opt.live_batch);
    }
    std::cerr << "usage \"" << config.usage << "\" is outside this engine's scope (supported: build, classify, target as an offline replay)" << std::endl;
    return 2;
}

// the value of an off|current|build option (RB_PASS_LISTS_*); false: none of the three
static bool lists_mode_arg(const char* v, int* out)
{
    if (!std::strcmp(v, "off")) *out = RB_PASS_LISTS_OFF;
    else if (!std::strcmp(v, "current")) *out = RB_PASS_LISTS_CURRENT;
    else if (!std::strcmp(v, "build")) *out = RB_PASS_LISTS_BUILD;
    else return false;
    return true;
}

int main(int argc, char const* argv[])
{
    std::string config_path;
    bool dump_only = false;
    IngestOptions opt;
    bool no_digest = false;
    std::vector<int> devices{0};
    std::string verify_path, verify_ref;
    uint64_t verify_fragment = 100000;  // [IBF] fragment_size default (configReader.cpp)
    std::string stats_path;
    double stats_error_rate = 0.1;  // [IBF] exp_seq_error_rate default (configReader.cpp); --error-rate
    EditOptions edit;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) {  // e.g. --devices 0,1,2,3,4,5,6,7
            devices.clear();
            std::string list = argv[++i];
            size_t pos = 0;
            while (pos <= list.size()) {
                const size_t comma = list.find(',', pos);
                const std::string tok = list.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
                if (!tok.empty()) devices.push_back(std::stoi(tok));
                if (comma == std::string::npos) break;
                pos = comma + 1;
            }
            if (devices.empty()) devices.push_back(0);
            continue;
        }
        if ((!std::strcmp(argv[i], "--config") || !std::strcmp(argv[i], "-c")) && i + 1 < argc) config_path = argv[++i];
        else if (!std::strcmp(argv[i], "--dump-config")) dump_only = true;
        else if (!std::strcmp(argv[i], "--verify-ibf") && i + 1 < argc) verify_path = argv[++i];
        else if (!std::strcmp(argv[i], "--reference") && i + 1 < argc) verify_ref = argv[++i];
        else if (!std::strcmp(argv[i], "--fragment-size") && i + 1 < argc) verify_fragment = (uint64_t)std::stoull(argv[++i]);
        else if (!std::strcmp(argv[i], "--no-digest")) no_digest = true;
        else if (!std::strcmp(argv[i], "--batch-reads") && i + 1 < argc) opt.batch_reads = std::max<size_t>(1, (size_t)std::stoull(argv[++i]));
        else if (!std::strcmp(argv[i], "--ingest-threads") && i + 1 < argc) opt.threads = (unsigned)std::max(1, std::stoi(argv[++i]));
        else if (!std::strcmp(argv[i], "--classify-threads") && i + 1 < argc) opt.classify_threads = (unsigned)std::max(1, std::stoi(argv[++i]));
        else if (!std::strcmp(argv[i], "--calibrate")) opt.calibrate = true;
        else if (!std::strcmp(argv[i], "--report-bins")) opt.report_bins = true;
        else if (!std::strcmp(argv[i], "--report-hits")) opt.report_hits = true;
        else if (!std::strcmp(argv[i], "--report-spans")) opt.report_spans = true;
        else if (!std::strcmp(argv[i], "--max-hits")) {
            char* end = nullptr;
            const unsigned long long v = i + 1 < argc ? std::strtoull(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || argv[i + 1][0] == '-' || *end != '\0' || v < 1 || v > (1ull << 20)) {
                std::cerr << "ERROR: --max-hits 1 .. 1048576" << std::endl;
                return 1;
            }
            opt.max_hits = (uint32_t)v;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--pass-lists")) {
            if (!lists_mode_arg(i + 1 < argc ? argv[i + 1] : "", &opt.pass_lists)) {
                std::cerr << "ERROR: --pass-lists off|current|build" << std::endl;
                return 1;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--wide-prefix-lists")) {
            if (!lists_mode_arg(i + 1 < argc ? argv[i + 1] : "", &opt.wide_prefix_lists)) {
                std::cerr << "ERROR: --wide-prefix-lists off|current|build" << std::endl;
                return 1;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--prefix-lists")) {
            if (!lists_mode_arg(i + 1 < argc ? argv[i + 1] : "", &opt.prefix_lists)) {
                std::cerr << "ERROR: --prefix-lists off|current|build" << std::endl;
                return 1;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--wide-lists")) {
            if (!lists_mode_arg(i + 1 < argc ? argv[i + 1] : "", &opt.wide_lists)) {
                std::cerr << "ERROR: --wide-lists off|current|build" << std::endl;
                return 1;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--wide-pass-lists")) {
            if (!lists_mode_arg(i + 1 < argc ? argv[i + 1] : "", &opt.wide_pass_lists)) {
                std::cerr << "ERROR: --wide-pass-lists off|current|build" << std::endl;
                return 1;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--report-prefixes")) opt.report_prefixes = true;
        else if (!std::strcmp(argv[i], "--prefix-lens")) {
            // a,b,c: 1 to 64 checkpoints in bases, none 0, strictly rising
            bool ok = i + 1 < argc && argv[i + 1][0] != '-' && argv[i + 1][0] != '\0' && opt.prefix_step == 0 && opt.prefix_count == 0 && opt.prefix_lens.empty();
            const char* s = ok ? argv[i + 1] : "";
            while (ok) {
                char* end = nullptr;
                const unsigned long long v = std::strtoull(s, &end, 10);
                ok = end != s && v >= 1 && v <= 0xFFFFFFFFull && (opt.prefix_lens.empty() || v > opt.prefix_lens.back()) && opt.prefix_lens.size() < RB_PREFIX_MAX &&
                     (*end == ',' || *end == '\0');
                if (!ok) break;
                opt.prefix_lens.push_back((uint32_t)v);
                if (*end == '\0') break;
                s = end + 1;
            }
            if (!ok) {
                std::cerr << "ERROR: --prefix-lens a,b,c: 1 to 64 checkpoints in bases, none 0, strictly rising; not together with --prefix-step / --prefix-count" << std::endl;
                return 1;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--prefix-step") || !std::strcmp(argv[i], "--prefix-count")) {
            const bool step = !std::strcmp(argv[i], "--prefix-step");
            char* end = nullptr;
            const unsigned long long v = i + 1 < argc ? std::strtoull(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || argv[i + 1][0] == '-' || *end != '\0' || v < 1 || v > (step ? 0xFFFFFFFFull : (unsigned long long)RB_PREFIX_MAX) || !opt.prefix_lens.empty()) {
                std::cerr << "ERROR: " << argv[i] << (step ? " N: bases between checkpoints, 1 or more" : " M: 1 to 64 checkpoints")
                          << "; --prefix-step / --prefix-count do not go together with --prefix-lens" << std::endl;
                return 1;
            }
            (step ? opt.prefix_step : opt.prefix_count) = (uint32_t)v;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--write-bin-map")) g_write_bin_map = true;
        else if (!std::strcmp(argv[i], "--edit-ibf") && i + 1 < argc) edit.input = argv[++i];
        else if (!std::strcmp(argv[i], "--with") && i + 1 < argc) edit.with.push_back(argv[++i]);
        else if (!std::strcmp(argv[i], "--output") && i + 1 < argc) edit.output = argv[++i];
        else if (!std::strcmp(argv[i], "--plan") && i + 1 < argc) edit.plan_path = argv[++i];
        else if (!std::strcmp(argv[i], "--drop-records") && i + 1 < argc) edit.drop_records = argv[++i];
        else if (!std::strcmp(argv[i], "--merge-every") && i + 1 < argc) {
            char* end = nullptr;
            edit.merge_every = std::strtoull(argv[++i], &end, 10);
            edit.merge_given = true;
            if (*end != '\0' || argv[i][0] == '-') { std::cerr << "ERROR: --merge-every N" << std::endl; return 1; }
        }
        else if (!std::strcmp(argv[i], "--filter-stats")) {  // with a file: the stand-alone report; bare (usage build): for every filter built
            g_filter_stats = true;
            if (i + 1 < argc && argv[i + 1][0] != '-') stats_path = argv[++i];
        }
        else if (!std::strcmp(argv[i], "--max-fp") && i + 1 < argc) g_stats_max_fp = std::stod(argv[++i]);
        else if (!std::strcmp(argv[i], "--chunk-length") && i + 1 < argc) g_stats_chunk_length = (uint32_t)std::stoul(argv[++i]);
        else if (!std::strcmp(argv[i], "--error-rate") && i + 1 < argc) stats_error_rate = std::stod(argv[++i]);
        else if (!std::strcmp(argv[i], "--bin-map") && i + 1 < argc) opt.bin_maps.push_back(argv[++i]);
        // tables of 1 GiB and more are placed by trial (up to five allocations probed, 1-2 s at load time): 1 switches it off
        else if (!std::strcmp(argv[i], "--placement-tries") && i + 1 < argc) {
            if (rb_set_placement_tries(std::stoi(argv[++i])) != RB_OK) { std::cerr << "ERROR: --placement-tries 0 .. 8" << std::endl; return 1; }
        }
        else if (!std::strcmp(argv[i], "--revcomp-of-n") && i + 1 < argc) interleave::set_revcomp_of_n((uint32_t)std::stoul(argv[++i]));
        else if (!std::strcmp(argv[i], "--mmap-output")) opt.mmap_output = true;
        else if (!std::strcmp(argv[i], "--no-mmap-output")) opt.mmap_output = false;
        else if (!std::strcmp(argv[i], "--segment-mb") && i + 1 < argc) opt.segment_mb = std::max<size_t>(1, (size_t)std::stoull(argv[++i]));
        else if (!std::strcmp(argv[i], "--segment-bytes") && i + 1 < argc) opt.segment_bytes = (size_t)std::stoull(argv[++i]);
        else if (!std::strcmp(argv[i], "--live-batch") && i + 1 < argc) opt.live_batch = std::max<size_t>(1, (size_t)std::stoull(argv[++i]));
        else if (!std::strcmp(argv[i], "--parse-stats") && i + 1 < argc) {
            // ingest self-check (no GPU): records, bases and an FNV-1a digest over "id\tseq\n" of every record
            seqio::MappedFile mf(argv[++i]);
            if (!mf.is_open()) { std::cerr << "ERROR: Unable to open the file: " << argv[i] << std::endl; return 1; }
            // through the parallel reader (--ingest-threads / --segment-bytes given BEFORE --parse-stats apply): the digest is
            // over the records in file order, so it is the same for every thread count and segment size
            uint64_t n = 0, bases = 0, h = 1469598103934665603ull;
            auto mix = [&](const char* d, size_t len) { for (size_t k = 0; k < len; ++k) { h ^= (unsigned char)d[k]; h *= 1099511628211ull; } };
            const auto t0 = std::chrono::steady_clock::now();
            seqio::ParallelReader reader(mf.data(), mf.size(), opt.threads, opt.bytes(), 0);
            const size_t n_segments = reader.segments();
            while (std::unique_ptr<seqio::Segment> seg = reader.next()) {
                for (const seqio::Record& r : seg->batch.records) {
                    ++n; bases += r.seq_len;
                    if (!no_digest) { mix(r.id, r.id_len); mix("\t", 1); mix(r.seq, r.seq_len); mix("\n", 1); }
                }
                if (!seg->batch.error.empty()) { std::cerr << "ERROR: " << seg->batch.error << std::endl; return 1; }
            }
            const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::cout << "records=" << n << " bases=" << bases << " fnv=" << h << " seconds=" << secs
                      << " MB_per_s=" << (secs > 0 ? mf.size() / 1e6 / secs : 0.0) << " segments=" << n_segments << std::endl;
            return 0;
        }
        else if (!std::strcmp(argv[i], "--help") || !std::strcmp(argv[i], "-h")) {
            std::cout << "readbouncer_amd --config <file.toml> [--dump-config] [--batch-reads N] [--ingest-threads N] [--classify-threads N] [--segment-mb N] [--mmap-output] [--calibrate] [--placement-tries N] [--revcomp-of-n 3|4] "
                         "[--devices 0,1,...] [--parse-stats file]\n"
                         "  usage build:    [--write-bin-map]  beside every <name>.ibf, <name>.bins.tsv: bin -> record id and fragment bounds\n"
                         "  usage classify: [--report-bins]  classified_bins.tsv: bin, strand, count and hit bins of every classified read\n"
                         "                  [--report-hits [--max-hits 64]]  classified_hits.tsv: every (bin, strand) at or above the threshold of those reads, with\n"
                         "                                    its count, at most --max-hits per (read, filter) (n_hits stays exact); bin_profile.tsv: reads per bin\n"
                         "                  [--pass-lists off|current|build]  --report-bins and --report-hits from a filter's list table: where it has a current one\n"
                         "                                    (current, the default), building one where it has none (build), or never (off); the files are the same bytes\n"
                         "                  [--report-spans]  classified_spans.tsv: where along the read the best bin of every matching filter matched, on its best\n"
                         "                                    strand: n_kmers, count, first, last, run_start, run_len, covered; positions in the read's coordinates\n"
                         "                  [--report-prefixes (--prefix-lens a,b,c | --prefix-step N [--prefix-count M])]  classified_prefixes.tsv: for EVERY read of the\n"
                         "                                    run, at each of up to 64 prefix checkpoints (bases, strictly rising; --prefix-step: N, 2N, ... M of them, default up\n"
                         "                                    to 1500 bases): prefix length, decision of the run's mode on that prefix, best target, every filter's maximum --\n"
                         "                                    from one pass over the read; prefix_summary.tsv: per checkpoint reads reaching it, with decision 0 / 1 / 2, first\n"
                         "                                    decided there, changed against the checkpoint before\n"
                         "                  [--prefix-lists off|current|build]  --report-prefixes from a filter's list table: never (off, the default), where it has a\n"
                         "                                    current one (current), or building one where it has none (build); the files are the same bytes\n"
                         "                  [--wide-prefix-lists off|current|build]  --report-prefixes from the wide list table of a filter of 8193 to 32256 bins:\n"
                         "                                    never (off, the default), where one is current (current; --wide-lists build makes one), or building it\n"
                         "                                    when the batch repays it (build); the files are the same bytes\n"
                         "                  [--wide-lists off|current|build]  count filters of 8193 to 32256 bins from their wide list table: never (off, the default),\n"
                         "                                    where one is current (current), or building it when the batch repays it (build); the files are the same bytes\n"
                         "                  [--bin-map <name>.bins.tsv ...]  adds the record id of the bin to these reports\n"
                         "                  [--filter-stats]  per-bin occupancy of every filter built: a summary and <name>.binstats.tsv (give the flag last, or\n"
                         "                                    before another flag: a bare word after it is taken as a file; a build's exit code stays 0 whatever the bins hold)\n"
                         "readbouncer_amd --verify-ibf <file.ibf> --reference <file.fasta> [--fragment-size N]\n"
                         "readbouncer_amd --filter-stats <file.ibf> [--bin-map <name>.bins.tsv] [--max-fp 0.01] [--chunk-length 360] [--error-rate 0.1]\n"
                         "                  bits, load, false-positive rate and estimated k-mers per bin -> <name>.binstats.tsv; exit code 3 when a bin is over --max-fp\n"
                         "readbouncer_amd --edit-ibf <a.ibf> [--with <b.ibf> ...] --output <out.ibf> (--plan <plan.tsv> | --merge-every N | --drop-records id[,id...])\n"
                         "                  [--bin-map <a.bins.tsv>[,<b.bins.tsv>...]] [--filter-stats]\n"
                         "                  a new filter whose bins are ORs of bins of the loaded ones, in HBM, without the FASTA; prints one EDIT_IBF line\n"
                         "                  --plan: rows out_bin<TAB>filter<TAB>bin (filter 0 = --edit-ibf, the --with files follow), # comments, `# bins=N` fixes the bin count\n"
                         "                  --merge-every N: out bin j = bins [jN, jN+N) of one filter; --drop-records (needs --bin-map): every bin of the other records, in order\n"
                         "                  --bin-map: also writes <out>.bins.tsv; --filter-stats: the report of the assembled table while it is in HBM (exit code 3)" << std::endl;
            return 0;
        }
    }
    if (opt.report_prefixes && opt.prefix_lens.empty()) {
        if (opt.prefix_step == 0) { std::cerr << "ERROR: --report-prefixes needs --prefix-lens a,b,c or --prefix-step N [--prefix-count M]" << std::endl; return 1; }
        // N, 2N, ...: M of them, by default as many as stay within the reference's 1500-base cut-off (at least one)
        const uint64_t m = opt.prefix_count ? opt.prefix_count : std::min<uint64_t>(RB_PREFIX_MAX, std::max<uint64_t>(1, 1500 / opt.prefix_step));
        for (uint64_t q = 1; q <= m && q * opt.prefix_step <= 0xFFFFFFFFull; ++q) opt.prefix_lens.push_back((uint32_t)(q * opt.prefix_step));
    }
    if (!verify_path.empty()) {
        if (verify_ref.empty()) { std::cerr << "ERROR: --verify-ibf <file.ibf> needs --reference <file.fasta> [--fragment-size N]" << std::endl; return 1; }
        try {
            return verify_ibf(verify_path, verify_ref, verify_fragment);
        } catch (const std::exception& e) {
            std::cerr << "ERROR: " << e.what() << std::endl;
            return 1;
        }
    }
    if (edit.input.empty() && (!edit.with.empty() || !edit.output.empty() || !edit.plan_path.empty() || edit.merge_given || !edit.drop_records.empty())) {
        std::cerr << "ERROR: --with, --output, --plan, --merge-every and --drop-records belong to --edit-ibf <a.ibf>" << std::endl;
        return 1;
    }
    if (!edit.input.empty()) {
        try {
            if (!stats_path.empty()) throw std::runtime_error("--edit-ibf: give --filter-stats without a file (last, or before another flag)");
            return edit_ibf(edit, opt.bin_maps, devices[0], g_filter_stats, stats_error_rate);
        } catch (const std::exception& e) {
            std::cerr << "ERROR: " << e.what() << std::endl;
            return 1;
        }
    }
    if (!stats_path.empty()) {
        try {
            interleave::IBFConfig cfg{};
            cfg.input_filter_file = stats_path;
            cfg.device = devices[0];
            interleave::IBF f{};
            f.load_filter(cfg);
            return filter_stats(f, stats_path, opt.bin_maps.empty() ? std::string() : opt.bin_maps[0], stats_error_rate);
        } catch (const std::exception& e) {
            std::cerr << "ERROR: " << e.what() << std::endl;
            return 1;
        }
    }
    if (config_path.empty()) {
        std::cerr << "ERROR: --config <file.toml> is required" << std::endl;
        return 1;
    }
    try {
        ConfigReader config(config_path);
        config.parse_general();
        if (dump_only) {
            config.parse();
            std::cout << config.dump();
            return 0;
        }
        // end-of-run report of main.cpp:438-444 (getrusage on Linux, main.cpp:140-152)
        const auto t_begin = std::chrono::steady_clock::now();
        const int rc = run_program(config, opt, devices);
        struct rusage ru;
        getrusage(RUSAGE_SELF, &ru);
        const double cpu = ru.ru_utime.tv_sec + ru.ru_stime.tv_sec + 1e-6 * (ru.ru_utime.tv_usec + ru.ru_stime.tv_usec);
        std::cout << "Real time : " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() << " sec" << std::endl;
        std::cout << "CPU time  : " << cpu << " sec" << std::endl;
        std::cout << "Peak RSS  : " << (int)((ru.ru_maxrss * 1024L) / (1024 * 1024)) << " MByte" << std::endl;
        return rc;
    } catch (const ConfigReaderException& e) {
        std::cerr << "Error in reading TOML configuration file!" << std::endl << e.what() << std::endl;
        return 1;
    } catch (const std::exception& e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        return 1;
    }
}
