# Prints the block of the reference's alg_data_trans_wrapper.cc that holds its six arithmetic functions: from the line
# that starts `float Fp16ToFp32(` up to, not including, the line `} // namespace ops_hccl`. The block is found by these
# text markers only. Every marker must occur exactly once in the file, and the six definitions must lie inside the
# block in the file's order; anything else ends with a message on stderr and exit status 1, which fails the build.
BEGIN {
    n = split("float Fp16ToFp32(|uint16_t Fp32DenormToFp16(|uint16_t Fp32ToFp16(|" \
              "HcclResult AicpuReduceFp16(|HcclResult AicpuReduce(|HcclResult AicpuReduceTemplate(", mark, "|")
    endmark = "} // namespace ops_hccl"
    next_mark = 1
}
{
    for (i = 1; i <= n; ++i) {
        if (index($0, mark[i]) == 1) {
            seen[i]++
            if (i == 1 && seen[i] == 1) {
                inside = 1
            }
            if (!inside || i != next_mark) {
                bad = bad sprintf("  line %d: `%s` outside the block or out of order\n", NR, mark[i])
            }
            next_mark = i + 1
        }
    }
    if (index($0, endmark) == 1) {
        ends++
        if (inside) {
            inside = 0
            closed++
        }
    }
    if (inside) {
        block = block $0 "\n"
    }
}
END {
    for (i = 1; i <= n; ++i) {
        if (seen[i] != 1) {
            bad = bad sprintf("  marker `%s` found %d times, expected once\n", mark[i], seen[i])
        }
    }
    if (ends != 1 || closed != 1) {
        bad = bad sprintf("  end marker `%s` found %d times (%d closing the block), expected once\n", endmark, ends, closed)
    }
    if (bad != "") {
        printf "extract_ref.awk: %s does not have the expected shape:\n%s", FILENAME, bad > "/dev/stderr"
        exit 1
    }
    printf "%s", block
}
